// Attention MAPS of the Vision Transformers: the probabilities that tia_mha_fwd_h (vit_attention.hip) never materialises, and the
// rollout recursion over them.  Neither kernel is on the path of a run that asks for no maps.
//
// tia_mha_probs_h:  p[b, h, i, j] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) for the first q_rows queries, float32, from the qkv
// Linear's own output [n, s, 3, heads, hd] (hd 64 or 80) -- per head, or the mean over the heads.
//
// One workgroup = (image, 64 queries, and one head or -- head_mean -- all of them in ascending order); each of its 4 waves owns 16
// query rows.  The product is tia_mha_fwd_h's first one, S^T = K Q^T on v_mfma_f32_16x16x32_f16 / _bf16: Q in registers as the B
// operand (lane l: query l & 15, dims 32 step + 8 (l >> 4) .. + 7), K in 64-key tiles through LDS as the A operand, so that
//   sc[kt][r] = score(query l & 15, key k0 + 16 kt + 4 (l >> 4) + r)
// and a query's 64 scores of a tile sit in the four lanes l & 15 (+ 16, 32, 48).  head_dim 80 is three k-steps whose dims 80..95 are
// exact zeros in both operands (lane quarters 2 and 3 of step 2 substitute a zero register).  All of that IS the forward's code:
// geometry, decode, Q load, K staging, score tile and online maximum come from vit_attention_tile.hpp, as mha_fwd_h_kernel's do.
//
// Two passes, so that no S-wide row has to live anywhere and s has no ceiling:
//   1. per head, the online maximum m and sum l of a query row over all key tiles (float32, base-2 domain: t = dot * scale * log2 e,
//      l = sum exp2(t - m), rescaled by exp2(m_old - m_new) when the maximum moves); (m, l) of every (head, query) go to LDS.
//   2. per key tile, for every head in ascending order: the scores again (the same score_tile on the same operands: the same
//      bits), p = exp2(t - m) / l -- ONE correctly rounded division, e_j / sum e rounded once -- and, with head_mean, acc += p in
//      float32 and acc / heads at the end.  The tile goes through LDS once (transposed so that a wave stores 64 consecutive floats
//      of a row) and is written once.  Nothing is accumulated in memory: no atomics, two launches agree bit for bit.
// Keys >= s are loaded as zeros and their t set to -inf before the maximum: exp2(-inf - m) = 0 exactly, and every tile the loops
// visit holds a real key, so m is finite from the first tile on.  Query rows >= q_rows compute on zeros and are not stored.
//
// tia_rollout_step_f32:  R_out = 1/2 (A R_in) + 1/2 R_in  on n float32 [s, s] matrices, v_mfma_f32_16x16x4_f32 (a k-ordered float32
// fma chain per output element: vit_f32.hip is the other user).  One workgroup = a 64 x 64 tile of one matrix, each wave 16 rows x
// 64 columns in four accumulators; A and R_in come in 32-deep k tiles through LDS, zero-filled beyond s (0 * 0 adds an exact zero),
// or -- R_in = I, d_r_in null -- R's tile is written as the identity's.  The epilogue halves both terms exactly and adds once.
//
// The rollout's other forms (max / min head fusion, a discard ratio; models/engine/_rollout_options.py states them) are siblings of
// these two: tia_mha_probs_fused_h is the probabilities kernel with another way of joining the heads (FUSE), tia_rollout_product_f32
// the step kernel without its blend (BLEND), and tia_rollout_discard_normalize_f32 a radix select per image (kth_smallest_kernel)
// in front of a row pass (discard_normalize_kernel).  A run with the default options launches none of them.
#include "vit_attention_tile.hpp"

namespace {

using namespace tia;
using namespace tia::mha;  // AT, KV_TILE, Geo, decode, load_q, stage_tile, score_tile, online_max: mha_fwd_h_kernel's own pieces

constexpr int T_PITCH = 68;   // floats per row of the transposed output tile (16-byte aligned rows)
constexpr int MAX_MEAN_HEADS = 64;  // head_mean keeps (m, l) of 64 queries per head in LDS: 512 bytes a head

// FUSE: what pass 2 does with the heads of a workgroup -- FUSE_SUM adds them (one head: 0 + p = p exactly; head_mean: / heads at the
// end), FUSE_MAX / FUSE_MIN keep the exact element-wise maximum / minimum of the SAME per-head values (head_mean geometry: one
// workgroup owns every head; nothing is divided).
constexpr int FUSE_SUM = 0, FUSE_MAX = 1, FUSE_MIN = 2;

template <bool BF, int HD, int FUSE>
__global__ __launch_bounds__(AT) void mha_probs_kernel(const unsigned short* __restrict__ qkv, float* __restrict__ out, int s, int heads,
                                                        int q_rows, int q_tiles, int head_mean, float scale_log2e) {
    using G = Geo<HD>;
    __shared__ __attribute__((aligned(16))) unsigned short k_lds[KV_TILE * G::PITCH];  // [key][dim]
    __shared__ __attribute__((aligned(16))) float t_lds[64 * T_PITCH];                 // [query][key]: the tile on its way out
    extern __shared__ float stat_lds[];                                                // [head of this workgroup][query][m, l]

    const Where w = decode(q_tiles);  // rest = (image, head), or -- head_mean -- the image
    const int tid = w.tid, lane = w.lane, wave = w.wave, r16 = w.r16, quarter = w.quarter, qt = w.qt, query = w.query;
    const int h0 = head_mean ? 0 : (int)(w.rest % heads);  // the first head of this workgroup, and how many it owns
    const int nh = head_mean ? heads : 1;
    const long b = head_mean ? w.rest : w.rest / heads;
    const long row_stride = 3L * heads * HD;  // halves between consecutive tokens of qkv
    const unsigned short* image = qkv + b * s * row_stride;

    // pass 1: the maximum and the sum of every (head, query) row
    for (int hl = 0; hl < nh; ++hl) {
        const unsigned short* base = image + (long)(h0 + hl) * HD;
        const unsigned short* kbase = base + (long)heads * HD;
        v4u qf[G::STEPS];
        load_q<HD>(base, row_stride, query, q_rows, quarter, qf);
        float m_run = -INFINITY, l_run = 0.0f;
        for (int k0 = 0; k0 < s; k0 += KV_TILE) {
            stage_tile<HD, false>(kbase, nullptr, row_stride, k0, s, tid, k_lds, nullptr);
            f32x4 t[4];
            const float t_max = score_tile<BF, HD>(k_lds, qf, k0, s, r16, quarter, scale_log2e, t);
            const float alpha = online_max(t_max, m_run);
            float p_sum = 0.0f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) p_sum += __builtin_amdgcn_exp2f(t[kt][r] - m_run);
            l_run = l_run * alpha + p_sum;
        }
        const float l_tot = row_sum(l_run);
        if (quarter == 0) {
            stat_lds[(hl * 64 + wave * 16 + r16) * 2] = m_run;
            stat_lds[(hl * 64 + wave * 16 + r16) * 2 + 1] = l_tot;
        }
    }
    __syncthreads();

    // pass 2: per key tile, every head's probabilities -- each output tile is written once
    const float count = (float)heads;
    for (int k0 = 0; k0 < s; k0 += KV_TILE) {
        f32x4 acc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const float first = FUSE == FUSE_MIN ? INFINITY : 0.0f;  // (every p is >= +0: max(0, p) = p)
            acc[kt] = f32x4{first, first, first, first};
        }
        for (int hl = 0; hl < nh; ++hl) {
            const unsigned short* base = image + (long)(h0 + hl) * HD;
            const unsigned short* kbase = base + (long)heads * HD;
            v4u qf[G::STEPS];
            load_q<HD>(base, row_stride, query, q_rows, quarter, qf);
            stage_tile<HD, false>(kbase, nullptr, row_stride, k0, s, tid, k_lds, nullptr);
            f32x4 t[4];
            score_tile<BF, HD>(k_lds, qf, k0, s, r16, quarter, scale_log2e, t);
            const float m = stat_lds[(hl * 64 + wave * 16 + r16) * 2], l = stat_lds[(hl * 64 + wave * 16 + r16) * 2 + 1];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (FUSE == FUSE_SUM) {
                        acc[kt][r] += __builtin_amdgcn_exp2f(t[kt][r] - m) / l;  // (one head: 0 + p = p exactly)
                    } else {
                        const float p = __builtin_amdgcn_exp2f(t[kt][r] - m) / l;
                        acc[kt][r] = FUSE == FUSE_MAX ? fmaxf(acc[kt][r], p) : fminf(acc[kt][r], p);
                    }
                }
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (FUSE == FUSE_SUM && head_mean) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[kt][r] = acc[kt][r] / count;
            }
            *reinterpret_cast<f32x4*>(&t_lds[(wave * 16 + r16) * T_PITCH + 16 * kt + 4 * quarter]) = acc[kt];
        }
        __syncthreads();  // (the next write of t_lds is two barriers away, behind the next tile's staging)
        const int key = k0 + lane;
#pragma unroll 4
        for (int qq = 0; qq < 16; ++qq) {
            const int q = qt * 64 + wave * 16 + qq;
            if (q < q_rows && key < s) {
                const long row = head_mean ? b * q_rows + q : (b * heads + h0) * q_rows + q;
                out[row * s + key] = t_lds[(wave * 16 + qq) * T_PITCH + lane];
            }
        }
    }
}

// ---- rollout step ---------------------------------------------------------------------------------------------------------------
constexpr int RT = 64;        // output tile: 64 x 64, a wave owns 16 rows
constexpr int RK = 32;        // k tile
constexpr int A_PITCH = 34;   // floats: lane (row r, k q) of a half wave reads bank 2 r + q -- 32 distinct
constexpr int R_PITCH = 80;   // floats: lane (k q, column c) of a half wave reads bank 16 q + c -- 32 distinct

// BLEND: the epilogue of tia_rollout_step_f32 (1/2 (A R) + 1/2 R); without it the product alone, R_out = A R (tia_rollout_product_f32)
template <bool BLEND>
__global__ __launch_bounds__(AT) void rollout_step_kernel(const float* __restrict__ a, const float* __restrict__ r_in, float* __restrict__ r_out,
                                                           int s, int tiles) {
    __shared__ float a_lds[RT * A_PITCH];  // [row][k]
    __shared__ float r_lds[RK * R_PITCH];  // [k][column]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, quarter = lane >> 4;
    const long bid = blockIdx.x;
    const int ct = (int)(bid % tiles), rt = (int)((bid / tiles) % tiles);
    const long b = bid / ((long)tiles * tiles);
    const long mat = b * s * s;
    const int row0 = rt * RT, col0 = ct * RT;

    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int k0 = 0; k0 < s; k0 += RK) {
        float av[8], rv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // A: row (tid >> 5) + 8 i, k tid & 31;  R: k (tid >> 6) + 4 i, column tid & 63
            const int row = row0 + (tid >> 5) + 8 * i, ka = k0 + (tid & 31);
            av[i] = (row < s && ka < s) ? a[mat + (long)row * s + ka] : 0.0f;
            const int kr = k0 + (tid >> 6) + 4 * i, col = col0 + (tid & 63);
            if (r_in)
                rv[i] = (kr < s && col < s) ? r_in[mat + (long)kr * s + col] : 0.0f;
            else
                rv[i] = (kr < s && kr == col) ? 1.0f : 0.0f;
        }
        __syncthreads();  // every wave has finished reading the previous tile
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a_lds[((tid >> 5) + 8 * i) * A_PITCH + (tid & 31)] = av[i];
            r_lds[((tid >> 6) + 4 * i) * R_PITCH + (tid & 63)] = rv[i];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < RK / 4; ++ks) {  // A operand: A[row l & 15][k l >> 4];  B operand: R[k l >> 4][column l & 15]
            const float af = a_lds[(wave * 16 + r16) * A_PITCH + 4 * ks + quarter];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, r_lds[(4 * ks + quarter) * R_PITCH + 16 * c + r16], acc[c], 0, 0, 0);
        }
    }
    // acc[c][r] = (A R)[row0 + 16 wave + 4 quarter + r][col0 + 16 c + (l & 15)]
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + wave * 16 + 4 * quarter + r, col = col0 + 16 * c + r16;
            if (row < s && col < s) {
                const long at = mat + (long)row * s + col;
                if constexpr (BLEND) {
                    const float prev = r_in ? r_in[at] : (row == col ? 1.0f : 0.0f);
                    r_out[at] = 0.5f * acc[c][r] + 0.5f * prev;  // both halvings exact: one rounding
                } else {
                    r_out[at] = acc[c][r];  // (R_in = I: a + 0 * x = a, the matrix itself)
                }
            }
        }
}

// ---- discard and normalise (tia_rollout_discard_normalize_f32) -------------------------------------------------------------------
// kth_smallest_kernel: one workgroup of 1024 threads per image finds the k-th smallest (1-based, duplicates counted) of its s * s
// float32 values.  They are finite and >= 0, so their bit patterns order as unsigned integers: a radix select from the top, digits
// of 12, 10 and 10 bits (the first one holds the exponent and four mantissa bits: probabilities of one magnitude still spread over
// some tens of counters).  Per digit: a histogram in LDS of the values that carry the digits chosen so far (integer atomic adds:
// the counts do not depend on their order), then one lane walks the cumulative counts to the bin that holds the rank.  Any bit
// pattern indexes inside the histogram, and the walks are bounded by the bins a lane owns.
constexpr int ST = 1024;        // threads of the selection
constexpr int SEL_BINS = 4096;  // counters: 2^12, the widest digit
constexpr int SEL_GROUP = ST / 64;  // threads whose bin sums one lane of wave 0 adds up

__global__ __launch_bounds__(ST) void kth_smallest_kernel(const float* __restrict__ f, float* __restrict__ v_out, long count, unsigned k) {
    __shared__ unsigned hist[SEL_BINS];
    __shared__ unsigned part[ST];  // a thread's bins added up
    __shared__ unsigned chosen[2];  // the bin that holds the rank, and the rank inside it

    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned* x = reinterpret_cast<const unsigned*>(f) + (long)blockIdx.x * count;
    unsigned prefix = 0u, mask = 0u, rank = k;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
        const int bins = pass == 0 ? SEL_BINS : 1024, per = bins / ST;
        for (int i = tid; i < SEL_BINS; i += ST) hist[i] = 0u;
        if (tid == 0) { chosen[0] = 0u; chosen[1] = 1u; }
        __syncthreads();
        for (long i = tid; i < count; i += ST) {
            const unsigned u = x[i];
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & (unsigned)(bins - 1)], 1u);
        }
        __syncthreads();
        unsigned mine = 0u;
        for (int i = 0; i < per; ++i) mine += hist[tid * per + i];
        part[tid] = mine;
        __syncthreads();
        if (tid < 64) {
            unsigned group = 0u;
            for (int i = 0; i < SEL_GROUP; ++i) group += part[lane * SEL_GROUP + i];
            unsigned incl = group;
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned o = __shfl_up(incl, off, 64);
                if (lane >= off) incl += o;
            }
            const unsigned excl = incl - group;
            if (rank > excl && rank <= incl) {  // one lane: 1 <= rank <= the number of values counted
                unsigned r = rank - excl;
                int t = lane * SEL_GROUP;
                while (t < lane * SEL_GROUP + SEL_GROUP - 1 && r > part[t]) r -= part[t++];
                int b = t * per;
                while (b < t * per + per - 1 && r > hist[b]) r -= hist[b++];
                chosen[0] = (unsigned)b;
                chosen[1] = r;
            }
        }
        __syncthreads();
        prefix |= chosen[0] << shift;
        mask |= (unsigned)(bins - 1) << shift;
        rank = chosen[1];
        __syncthreads();  // (chosen and hist are rewritten by the next digit)
    }
    if (tid == 0) v_out[blockIdx.x] = __uint_as_float(prefix);
}

// discard_normalize_kernel: one wave per row i of one image.  A^[i][j] = ((F'[i][j] + [i == j]) / 2) / s_i with F' = F, but 0 where
// F <= v and (i, j) != (0, 0) (has_v), and s_i the row sum in THIS order: lane l adds its entries j = l, l + 64, ... in ascending
// order to 0, then the 64 partial sums fold by the exchange tree p[l] += p[l ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 (every lane ends with
// the same bits: the additions of a level commute).  The row is read twice and written once; s_i >= 1/2.
__device__ __forceinline__ float halved_entry(float x, float thr, bool has_v, bool origin, bool diagonal) {
    const float kept = (has_v && x <= thr && !origin) ? 0.0f : x;
    return 0.5f * (kept + (diagonal ? 1.0f : 0.0f));
}

__global__ __launch_bounds__(AT) void discard_normalize_kernel(const float* __restrict__ f, const float* __restrict__ v, float* __restrict__ out,
                                                                int s, int has_v, long rows) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * 4 + wave;  // of all n * s rows
    if (row >= rows) return;                       // (a whole wave: nothing below is a workgroup barrier)
    const long b = row / s;
    const int i = (int)(row - b * s);
    const float thr = has_v ? v[b] : 0.0f;
    const float* src = f + row * s;
    float* dst = out + row * s;
    float sum = 0.0f;
    for (int j = lane; j < s; j += 64) sum += halved_entry(src[j], thr, has_v != 0, (i | j) == 0, i == j);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    for (int j = lane; j < s; j += 64) dst[j] = halved_entry(src[j], thr, has_v != 0, (i | j) == 0, i == j) / sum;
}

bool overlap(const void* p, uint64_t p_bytes, const void* q, uint64_t q_bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + q_bytes && b < a + p_bytes;
}

bool overlap(const void* p, const void* q, uint64_t bytes) { return overlap(p, bytes, q, bytes); }

// the checks and the launch of both forms of the probabilities kernel: q_rows queries per head or head mean (FUSE_SUM), or all rows
// with the heads' maximum / minimum
int launch_probs(const void* d_qkv, float* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale, int64_t q_rows,
                 int32_t head_mean, int fuse, int32_t dtype, void* stream) {
    // (own checks around the shared ones: the first stands among check_args's leading TIA_EINVALs, the last among its trailing TIA_ESIZEs)
    if (q_rows < 1 || q_rows > s || (head_mean != 0 && head_mean != 1)) return TIA_EINVAL;
    const long groups = head_mean ? 1 : heads;  // workgroups per (image, query tile)
    long q_tiles;
    const int code = check_args(d_qkv, d_out, n, s, heads, head_dim, scale, dtype == TIA_DT_F16 || dtype == TIA_DT_BF16, q_rows, groups, &q_tiles);
    if (code != TIA_OK) return code;
    if (head_mean && heads > MAX_MEAN_HEADS) return TIA_ESIZE;
    const long blocks = n * groups * q_tiles;
    const size_t stat_bytes = (size_t)(head_mean ? heads : 1) * 64 * 2 * sizeof(float);
    const float scale_log2e = scale * 1.44269504088896340736f;
    const bool bf = dtype == TIA_DT_BF16;
    auto kernel = head_dim == 80 ? (bf ? mha_probs_kernel<true, 80, FUSE_SUM> : mha_probs_kernel<false, 80, FUSE_SUM>)
                                 : (bf ? mha_probs_kernel<true, 64, FUSE_SUM> : mha_probs_kernel<false, 64, FUSE_SUM>);
    if (fuse == FUSE_MAX)
        kernel = head_dim == 80 ? (bf ? mha_probs_kernel<true, 80, FUSE_MAX> : mha_probs_kernel<false, 80, FUSE_MAX>)
                                : (bf ? mha_probs_kernel<true, 64, FUSE_MAX> : mha_probs_kernel<false, 64, FUSE_MAX>);
    else if (fuse == FUSE_MIN)
        kernel = head_dim == 80 ? (bf ? mha_probs_kernel<true, 80, FUSE_MIN> : mha_probs_kernel<false, 80, FUSE_MIN>)
                                : (bf ? mha_probs_kernel<true, 64, FUSE_MIN> : mha_probs_kernel<false, 64, FUSE_MIN>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(AT), stat_bytes, (hipStream_t)stream, (const unsigned short*)d_qkv, d_out,
                       (int)s, (int)heads, (int)q_rows, (int)q_tiles, (int)head_mean, scale_log2e);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

// the checks and the launch of both epilogues of the rollout matrix product
template <bool BLEND>
int launch_rollout(const float* d_a, const float* d_r_in, float* d_r_out, int64_t n, int64_t s, void* stream) {
    if (!d_a || !d_r_out || n <= 0 || s <= 0) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_r_in) | reinterpret_cast<uintptr_t>(d_r_out)) & 3) return TIA_EINVAL;
    if (s > 0x7fffffffL - RT) return TIA_ESIZE;
    const long tiles = (s + RT - 1) / RT;
    if (tiles > 46340 || n > 0x7fffffffL / (tiles * tiles)) return TIA_ESIZE;  // one grid dimension
    if (n > INT64_MAX / 4 / s / s) return TIA_ESIZE;
    const uint64_t bytes = (uint64_t)n * s * s * sizeof(float);
    if (overlap(d_r_out, d_a, bytes) || (d_r_in && overlap(d_r_out, d_r_in, bytes))) return TIA_EINVAL;
    hipLaunchKernelGGL(rollout_step_kernel<BLEND>, dim3((unsigned)(n * tiles * tiles)), dim3(AT), 0, (hipStream_t)stream, d_a, d_r_in,
                       d_r_out, (int)s, (int)tiles);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

}  // namespace

extern "C" int tia_mha_probs_h(const void* d_qkv, float* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale,
                               int64_t q_rows, int32_t head_mean, int32_t dtype, void* stream) {
    return launch_probs(d_qkv, d_out, n, s, heads, head_dim, scale, q_rows, head_mean, FUSE_SUM, dtype, stream);
}

extern "C" int tia_mha_probs_fused_h(const void* d_qkv, float* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale,
                                     int32_t fusion, int32_t dtype, void* stream) {
    if (fusion != TIA_FUSE_MEAN && fusion != TIA_FUSE_MAX && fusion != TIA_FUSE_MIN) return TIA_EINVAL;
    const int fuse = fusion == TIA_FUSE_MAX ? FUSE_MAX : (fusion == TIA_FUSE_MIN ? FUSE_MIN : FUSE_SUM);
    return launch_probs(d_qkv, d_out, n, s, heads, head_dim, scale, s, 1, fuse, dtype, stream);
}

extern "C" int tia_rollout_step_f32(const float* d_a, const float* d_r_in, float* d_r_out, int64_t n, int64_t s, void* stream) {
    return launch_rollout<true>(d_a, d_r_in, d_r_out, n, s, stream);
}

extern "C" int tia_rollout_product_f32(const float* d_a, const float* d_r_in, float* d_r_out, int64_t n, int64_t s, void* stream) {
    return launch_rollout<false>(d_a, d_r_in, d_r_out, n, s, stream);
}

extern "C" int tia_rollout_discard_normalize_f32(const float* d_f, float* d_out, float* d_v, int64_t n, int64_t s, int64_t k, void* stream) {
    if (!d_f || !d_out || n <= 0 || s <= 0 || k < 0 || (k > 0 && !d_v)) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_f) | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_v)) & 3) return TIA_EINVAL;
    if (s > 0xffff) return TIA_ESIZE;  // s * s < 2^32: the selection counts in 32 bits
    if (k >= s * s) return TIA_EINVAL;
    if (n > 0x7fffffffL || n > INT64_MAX / 4 / s / s) return TIA_ESIZE;
    const long rows = n * s, blocks = (rows + 3) / 4;
    if (blocks > 0x7fffffffL) return TIA_ESIZE;  // one grid dimension
    const uint64_t bytes = (uint64_t)n * s * s * sizeof(float), v_bytes = (uint64_t)n * sizeof(float);
    if (overlap(d_out, d_f, bytes)) return TIA_EINVAL;
    if (k > 0 && (overlap(d_v, v_bytes, d_f, bytes) || overlap(d_v, v_bytes, d_out, bytes))) return TIA_EINVAL;
    if (k > 0) {
        hipLaunchKernelGGL(kth_smallest_kernel, dim3((unsigned)n), dim3(ST), 0, (hipStream_t)stream, d_f, d_v, (long)(s * s), (unsigned)k);
        if (hipGetLastError() != hipSuccess) return TIA_ELAUNCH;
    }
    hipLaunchKernelGGL(discard_normalize_kernel, dim3((unsigned)blocks), dim3(AT), 0, (hipStream_t)stream, d_f, (const float*)d_v, d_out,
                       (int)s, (int)(k > 0), rows);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
