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
// exact zeros in both operands (lane quarters 2 and 3 of step 2 substitute a zero register), as in mha_fwd_h80_kernel.
//
// Two passes, so that no S-wide row has to live anywhere and s has no ceiling:
//   1. per head, the online maximum m and sum l of a query row over all key tiles (float32, base-2 domain: t = dot * scale * log2 e,
//      l = sum exp2(t - m), rescaled by exp2(m_old - m_new) when the maximum moves); (m, l) of every (head, query) go to LDS.
//   2. per key tile, for every head in ascending order: the scores again (the same instructions on the same operands: the same
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
#include "conv_device.hpp"
#include "wide_io.hpp"

namespace {

using namespace tia;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int AT = 256;       // threads: 4 waves x 16 query rows
constexpr int KV_TILE = 64;   // keys per LDS tile
constexpr int T_PITCH = 68;   // floats per row of the transposed output tile (16-byte aligned rows)
constexpr int MAX_MEAN_HEADS = 64;  // head_mean keeps (m, l) of 64 queries per head in LDS: 512 bytes a head

template <bool BF>
__device__ __forceinline__ f32x4 mma16(const v4u& a, const v4u& b, const f32x4& c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const b8*>(&a), *reinterpret_cast<const b8*>(&b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(&a), *reinterpret_cast<const h8*>(&b), c, 0, 0, 0);
}

// HD 64: rows of 64 + 8 halves (the pitch of mha_fwd_h_kernel); HD 80: 80, conflict-free without a pad (mha_fwd_h80_kernel's count)
template <int HD>
struct Geo {
    static constexpr int PITCH = HD == 64 ? 72 : 80;
    static constexpr int STEPS = HD == 64 ? 2 : 3;
    static constexpr int VEC = HD / 8;                          // 16-byte vectors per row
    static constexpr int ROUNDS = (KV_TILE * VEC + AT - 1) / AT;  // staging rounds of the workgroup
};

template <int HD>
__device__ __forceinline__ void load_q(const unsigned short* base, long row_stride, int query, int q_rows, int quarter,
                                       v4u (&qf)[Geo<HD>::STEPS]) {
    const v4u zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int st = 0; st < Geo<HD>::STEPS; ++st) {
        const bool real = query < q_rows && 32 * st + 8 * quarter < HD;
        qf[st] = real ? *reinterpret_cast<const v4u*>(base + (long)query * row_stride + 32 * st + 8 * quarter) : zero4;
    }
}

// keys k0 .. k0 + 63 of one head into k_lds ([key][dim]), zeros beyond s; both barriers are inside
template <int HD>
__device__ __forceinline__ void stage_keys(const unsigned short* kbase, long row_stride, int k0, int s, int tid, unsigned short* k_lds) {
    using G = Geo<HD>;
    const v4u zero4 = {0u, 0u, 0u, 0u};
    v4u kreg[G::ROUNDS];
#pragma unroll
    for (int i = 0; i < G::ROUNDS; ++i) {
        const int v = tid + AT * i, row = v / G::VEC, c = v % G::VEC, key = k0 + row;
        kreg[i] = (v < KV_TILE * G::VEC && key < s) ? *reinterpret_cast<const v4u*>(kbase + (long)key * row_stride + 8 * c) : zero4;
    }
    __syncthreads();  // every wave has finished reading the previous tile
#pragma unroll
    for (int i = 0; i < G::ROUNDS; ++i) {
        const int v = tid + AT * i, row = v / G::VEC, c = v % G::VEC;
        if (v < KV_TILE * G::VEC) *reinterpret_cast<v4u*>(&k_lds[row * G::PITCH + 8 * c]) = kreg[i];
    }
    __syncthreads();
}

// t[kt][r] = scale * log2 e * score(query l & 15, key k0 + 16 kt + 4 quarter + r), -inf for keys >= s
template <bool BF, int HD>
__device__ __forceinline__ void score_tile(const unsigned short* k_lds, const v4u (&qf)[Geo<HD>::STEPS], int k0, int s, int r16, int quarter,
                                           float scale_log2e, f32x4 (&t)[4]) {
    using G = Geo<HD>;
    const v4u zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int st = 0; st < G::STEPS; ++st) {
            // (HD 80, step 2: quarters 2 and 3 are dims 80..95 -- they read the address of quarter & 1 and substitute zeros)
            const int q_read = 32 * st + 8 * quarter < HD ? quarter : (quarter & 1);
            v4u a = *reinterpret_cast<const v4u*>(&k_lds[(16 * kt + r16) * G::PITCH + 32 * st + 8 * q_read]);
            if (32 * st + 8 * quarter >= HD) a = zero4;
            acc = mma16<BF>(a, qf[st], acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + 16 * kt + 4 * quarter + r;
            t[kt][r] = key < s ? acc[r] * scale_log2e : -INFINITY;
        }
    }
}

template <bool BF, int HD>
__global__ __launch_bounds__(AT) void mha_probs_kernel(const unsigned short* __restrict__ qkv, float* __restrict__ out, int s, int heads,
                                                        int q_rows, int q_tiles, int head_mean, float scale_log2e) {
    using G = Geo<HD>;
    __shared__ __attribute__((aligned(16))) unsigned short k_lds[KV_TILE * G::PITCH];  // [key][dim]
    __shared__ __attribute__((aligned(16))) float t_lds[64 * T_PITCH];                 // [query][key]: the tile on its way out
    extern __shared__ float stat_lds[];                                                // [head of this workgroup][query][m, l]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, quarter = lane >> 4;
    const long bid = blockIdx.x;
    const int qt = (int)(bid % q_tiles);
    const long rest = bid / q_tiles;
    const int h0 = head_mean ? 0 : (int)(rest % heads);  // the first head of this workgroup, and how many it owns
    const int nh = head_mean ? heads : 1;
    const long b = head_mean ? rest : rest / heads;
    const long row_stride = 3L * heads * HD;  // halves between consecutive tokens of qkv
    const unsigned short* image = qkv + b * s * row_stride;
    const int query = qt * 64 + wave * 16 + r16;

    // pass 1: the maximum and the sum of every (head, query) row
    for (int hl = 0; hl < nh; ++hl) {
        const unsigned short* base = image + (long)(h0 + hl) * HD;
        const unsigned short* kbase = base + (long)heads * HD;
        v4u qf[G::STEPS];
        load_q<HD>(base, row_stride, query, q_rows, quarter, qf);
        float m_run = -INFINITY, l_run = 0.0f;  // l_run: this lane's share of the row sum (its 16 keys per tile)
        for (int k0 = 0; k0 < s; k0 += KV_TILE) {
            stage_keys<HD>(kbase, row_stride, k0, s, tid, k_lds);
            f32x4 t[4];
            score_tile<BF, HD>(k_lds, qf, k0, s, r16, quarter, scale_log2e, t);
            float t_max = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) t_max = fmaxf(t_max, t[kt][r]);
            t_max = fmaxf(t_max, __shfl_xor(t_max, 16, 64));
            t_max = fmaxf(t_max, __shfl_xor(t_max, 32, 64));
            const float m_new = fmaxf(m_run, t_max);                    // finite: the tile holds a real key
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0
            m_run = m_new;
            float p_sum = 0.0f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) p_sum += __builtin_amdgcn_exp2f(t[kt][r] - m_new);
            l_run = l_run * alpha + p_sum;
        }
        float l_tot = l_run + __shfl_xor(l_run, 16, 64);
        l_tot += __shfl_xor(l_tot, 32, 64);
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
        for (int kt = 0; kt < 4; ++kt) acc[kt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int hl = 0; hl < nh; ++hl) {
            const unsigned short* base = image + (long)(h0 + hl) * HD;
            const unsigned short* kbase = base + (long)heads * HD;
            v4u qf[G::STEPS];
            load_q<HD>(base, row_stride, query, q_rows, quarter, qf);
            stage_keys<HD>(kbase, row_stride, k0, s, tid, k_lds);
            f32x4 t[4];
            score_tile<BF, HD>(k_lds, qf, k0, s, r16, quarter, scale_log2e, t);
            const float m = stat_lds[(hl * 64 + wave * 16 + r16) * 2], l = stat_lds[(hl * 64 + wave * 16 + r16) * 2 + 1];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[kt][r] += __builtin_amdgcn_exp2f(t[kt][r] - m) / l;  // (one head: 0 + p = p exactly)
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (head_mean) {
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
                const float prev = r_in ? r_in[at] : (row == col ? 1.0f : 0.0f);
                r_out[at] = 0.5f * acc[c][r] + 0.5f * prev;  // both halvings exact: one rounding
            }
        }
}

bool overlap(const void* p, const void* q, uint64_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + bytes && b < a + bytes;
}

}  // namespace

extern "C" int tia_mha_probs_h(const void* d_qkv, float* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale,
                               int64_t q_rows, int32_t head_mean, int32_t dtype, void* stream) {
    if (!d_qkv || !d_out || n <= 0 || s <= 0 || heads <= 0 || head_dim <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (!(scale > 0.0f) || !(scale < INFINITY)) return TIA_EINVAL;
    if (q_rows < 1 || q_rows > s || (head_mean != 0 && head_mean != 1)) return TIA_EINVAL;
    if (head_dim != 64 && head_dim != 80) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_qkv) | reinterpret_cast<uintptr_t>(d_out)) & 15) return TIA_EINVAL;
    if (s > 0x7fffffffL - KV_TILE || heads > 0x7fffffffL / (3 * head_dim)) return TIA_ESIZE;
    if (head_mean && heads > MAX_MEAN_HEADS) return TIA_ESIZE;
    const long q_tiles = (q_rows + 63) / 64;
    const long groups = head_mean ? 1 : heads;  // workgroups per (image, query tile)
    if (n > 0x7fffffffL / groups || n * groups > 0x7fffffffL / q_tiles) return TIA_ESIZE;  // one grid dimension
    const long blocks = n * groups * q_tiles;
    const size_t stat_bytes = (size_t)(head_mean ? heads : 1) * 64 * 2 * sizeof(float);
    const float scale_log2e = scale * 1.44269504088896340736f;
    const bool bf = dtype == TIA_DT_BF16;
    const auto kernel = head_dim == 80 ? (bf ? mha_probs_kernel<true, 80> : mha_probs_kernel<false, 80>)
                                       : (bf ? mha_probs_kernel<true, 64> : mha_probs_kernel<false, 64>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(AT), stat_bytes, (hipStream_t)stream, (const unsigned short*)d_qkv, d_out,
                       (int)s, (int)heads, (int)q_rows, (int)q_tiles, (int)head_mean, scale_log2e);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_rollout_step_f32(const float* d_a, const float* d_r_in, float* d_r_out, int64_t n, int64_t s, void* stream) {
    if (!d_a || !d_r_out || n <= 0 || s <= 0) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_a) | reinterpret_cast<uintptr_t>(d_r_in) | reinterpret_cast<uintptr_t>(d_r_out)) & 3) return TIA_EINVAL;
    if (s > 0x7fffffffL - RT) return TIA_ESIZE;
    const long tiles = (s + RT - 1) / RT;
    if (tiles > 46340 || n > 0x7fffffffL / (tiles * tiles)) return TIA_ESIZE;  // one grid dimension
    if (n > INT64_MAX / 4 / s / s) return TIA_ESIZE;
    const uint64_t bytes = (uint64_t)n * s * s * sizeof(float);
    if (overlap(d_r_out, d_a, bytes) || (d_r_in && overlap(d_r_out, d_r_in, bytes))) return TIA_EINVAL;
    hipLaunchKernelGGL(rollout_step_kernel, dim3((unsigned)(n * tiles * tiles)), dim3(AT), 0, (hipStream_t)stream, d_a, d_r_in, d_r_out,
                       (int)s, (int)tiles);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
