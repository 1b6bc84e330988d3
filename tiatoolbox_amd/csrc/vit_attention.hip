// Fused multi-head attention forward for the Vision Transformers (fp16 / bf16, head_dim 64; the 80 form is further down), on v_mfma_f32_16x16x32_f16 / _bf16:
//   out[b, i, h, :] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) @ v[b, :, h, :]
// on the qkv Linear's own output order [n, s, 3, heads, 64] (no permute pass), written as [n, s, heads * 64].
//
// One workgroup = (image, head, 64 queries); each of its 4 waves owns 16 query rows, whose Q stays in registers as the B operand
// (lane l: query l & 15, dims 32 step + 8 (l >> 4) .. + 7: one 16-byte global load per step).  K and V come in 64-key tiles through
// LDS.  The first product is the SWAPPED one, S^T = K Q^T: A = K (row = key), so the accumulator of key group kt holds
//   sc[kt][r] = score(query l & 15, key 16 kt + 4 (l >> 4) + r)
// -- a query's 64 scores of a tile sit in the 16 registers of the four lanes l & 15, l & 15 + 16, + 32, + 48.  Row maximum and row sum are
// 15 register operations and two lane exchanges; the running maximum m and the sum l live in the lane of their query.
// The second product is O^T = V^T P^T with B = P^T: the rounded accumulators ARE that operand, with no lane movement and no LDS:
// element j of lane quarter q in k-step s2 is key 32 s2 + 16 (j >> 2) + 4 q + (j & 3).  V is therefore written to LDS transposed
// ([dim][key]) with the keys of a row in exactly that order (key_slot below), so that the A operand (row = dim 16 db + (l & 15))
// is one 16-byte LDS read.  O^T's accumulator has the query on the lane again (o[db][r] = O[query l & 15][dim 16 db + 4 (l >> 4) + r]),
// so the rescale by exp2(m_old - m_new) and the final 1 / l need no exchange either.
//
// Arithmetic: float32 online softmax in the base-2 domain (t = dot * scale * log2 e); the sum is taken over the unrounded float32 p, p is
// rounded once to the half type for the MFMA, the output O / l is rounded once.  Keys >= s are loaded as zeros and their scores set
// to -inf BEFORE the maximum: p = exp2(-inf - m) = 0 exactly, and since every tile the loop visits holds at least one real key
// (k0 < s) the new maximum is finite from the first tile on: m_old - m_new is -inf - finite there, never inf - inf.  Query rows >= s
// compute on zeros and are not stored.
#include "conv_device.hpp"
#include "wide_io.hpp"

namespace {

using namespace tia;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int AT = 256;       // threads: 4 waves x 16 query rows
constexpr int KV_TILE = 64;   // keys per LDS tile
constexpr int HEAD_DIM = 64;
constexpr int PITCH = 72;     // halves per LDS row: 64 + 8 (144 bytes: 16-byte aligned rows, 16-byte reads of 16 rows spread over the banks)

template <bool BF>
__device__ __forceinline__ f32x4 mma16(const v4u& a, const v4u& b, const f32x4& c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const b8*>(&a), *reinterpret_cast<const b8*>(&b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(&a), *reinterpret_cast<const h8*>(&b), c, 0, 0, 0);
}

// where key `row` of a tile sits in a row of the transposed V image: the k order of the P^T operand (see above)
__device__ __forceinline__ int key_slot(int row) {
    const int kk = row & 31;
    return (row & 32) + 8 * ((kk >> 2) & 3) + 4 * (kk >> 4) + (kk & 3);
}

template <bool BF>
__global__ __launch_bounds__(AT) void mha_fwd_h_kernel(const unsigned short* __restrict__ qkv, unsigned short* __restrict__ out, int s,
                                                        int heads, int q_tiles, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) unsigned short k_lds[KV_TILE * PITCH];   // [key][dim]
    __shared__ __attribute__((aligned(16))) unsigned short vt_lds[HEAD_DIM * PITCH];  // [dim][key slot]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, quarter = lane >> 4;
    const long bid = blockIdx.x;
    const int qt = (int)(bid % q_tiles);
    const long bh = bid / q_tiles;
    const int head = (int)(bh % heads);
    const long b = bh / heads;
    const long row_stride = 3L * heads * HEAD_DIM;  // halves between consecutive tokens of qkv
    const unsigned short* base = qkv + b * s * row_stride + (long)head * HEAD_DIM;
    const unsigned short* kbase = base + (long)heads * HEAD_DIM;
    const unsigned short* vbase = base + 2L * heads * HEAD_DIM;

    const v4u zero4 = {0u, 0u, 0u, 0u};
    const int query = qt * 64 + wave * 16 + r16;
    v4u qf[2];
#pragma unroll
    for (int st = 0; st < 2; ++st)
        qf[st] = query < s ? *reinterpret_cast<const v4u*>(base + (long)query * row_stride + 32 * st + 8 * quarter) : zero4;

    f32x4 o[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m_run = -INFINITY, l_run = 0.0f;  // l_run: this lane's share of the row sum (its 16 keys per tile)

    for (int k0 = 0; k0 < s; k0 += KV_TILE) {
        // this thread's part of the tile: rows (tid >> 3) and (tid >> 3) + 32, dims 8 (tid & 7) .. + 7
        v4u kreg[2], vreg[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (tid >> 3) + 32 * i, key = k0 + row;
            const long off = (long)key * row_stride + 8 * (tid & 7);
            kreg[i] = key < s ? *reinterpret_cast<const v4u*>(kbase + off) : zero4;
            vreg[i] = key < s ? *reinterpret_cast<const v4u*>(vbase + off) : zero4;
        }
        __syncthreads();  // every wave has finished reading the previous tile
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (tid >> 3) + 32 * i, c8 = tid & 7;
            *reinterpret_cast<v4u*>(&k_lds[row * PITCH + 8 * c8]) = kreg[i];
            const int slot = key_slot(row);
            const unsigned w[4] = {vreg[i].x, vreg[i].y, vreg[i].z, vreg[i].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                vt_lds[(8 * c8 + 2 * e) * PITCH + slot] = (unsigned short)(w[e] & 0xffffu);
                vt_lds[(8 * c8 + 2 * e + 1) * PITCH + slot] = (unsigned short)(w[e] >> 16);
            }
        }
        __syncthreads();

        // S^T = K Q^T: 4 key groups x 2 steps over the 64 dims
        f32x4 sc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const v4u a = *reinterpret_cast<const v4u*>(&k_lds[(16 * kt + r16) * PITCH + 32 * st + 8 * quarter]);
                acc = mma16<BF>(a, qf[st], acc);
            }
            sc[kt] = acc;
        }
        float t_max = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * kt + 4 * quarter + r;
                const float t = key < s ? sc[kt][r] * scale_log2e : -INFINITY;
                sc[kt][r] = t;
                t_max = fmaxf(t_max, t);
            }
        t_max = fmaxf(t_max, __shfl_xor(t_max, 16, 64));
        t_max = fmaxf(t_max, __shfl_xor(t_max, 32, 64));
        const float m_new = fmaxf(m_run, t_max);            // finite: the tile holds a real key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0
        m_run = m_new;
        float p_sum = 0.0f;
        unsigned short ph[4][4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(sc[kt][r] - m_new);
                p_sum += p;
                ph[kt][r] = f32_to_half<BF>(p);
            }
        l_run = l_run * alpha + p_sum;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[db][r] *= alpha;

        // O^T += V^T P^T: k-step s2 takes key groups 2 s2 (elements 0..3) and 2 s2 + 1 (elements 4..7)
        v4u pf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            pf[s2].x = (unsigned)ph[2 * s2][0] | ((unsigned)ph[2 * s2][1] << 16);
            pf[s2].y = (unsigned)ph[2 * s2][2] | ((unsigned)ph[2 * s2][3] << 16);
            pf[s2].z = (unsigned)ph[2 * s2 + 1][0] | ((unsigned)ph[2 * s2 + 1][1] << 16);
            pf[s2].w = (unsigned)ph[2 * s2 + 1][2] | ((unsigned)ph[2 * s2 + 1][3] << 16);
        }
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const v4u a = *reinterpret_cast<const v4u*>(&vt_lds[(16 * db + r16) * PITCH + 32 * s2 + 8 * quarter]);
                o[db] = mma16<BF>(a, pf[s2], o[db]);
            }
    }

    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    if (query < s) {
        unsigned short* op = out + ((long)b * s + query) * ((long)heads * HEAD_DIM) + (long)head * HEAD_DIM + 4 * quarter;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            uint2 w;
            w.x = (unsigned)f32_to_half<BF>(o[db][0] / l_tot) | ((unsigned)f32_to_half<BF>(o[db][1] / l_tot) << 16);
            w.y = (unsigned)f32_to_half<BF>(o[db][2] / l_tot) | ((unsigned)f32_to_half<BF>(o[db][3] / l_tot) << 16);
            *reinterpret_cast<uint2*>(op + 16 * db) = w;
        }
    }
}

// ---- head_dim 80 (Virchow / Virchow2: 1280 / 16) ---------------------------------------------------------------------------------
// The same workgroup, operand order and softmax as above; what 80 dimensions change:
//  * First product: k = 80 is 2.5 steps of the 16x16x32 MFMA, run as three steps whose dims 80..95 are exact zeros in BOTH operands.
//    Those dims are lane quarters 2 and 3 of step 2.  For Q such a lane keeps a zero register; for K it reads a real address (the
//    row's dims 64 + 8 (quarter & 1), so that every lane of the wave issues the same read) and then SUBSTITUTES the zero register: no
//    LDS pad column exists, so none can hold stale or uninitialised bits (0 x NaN would be NaN), and LDS has no 96-wide rows to pay for.
//  * Second product: 80 output dims are five 16-row blocks (o[5]), no padding; vt_lds has 80 rows.
//  * A tile is 64 rows x 10 sixteen-byte vectors per operand = 640 = 2.5 per thread: three rounds, the last one guarded.
//  * LDS row pitch 80 halves (160 bytes) for both images.  ds_read_b128 banks are (byte address / 4) mod 64 and conflicts count inside
//    four 16-lane groups, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: a group holds rows {0-3, 12-15} of one lane
//    quarter and rows {4-11} of the next, all 16 rows once.  In 16-byte slots (16 per 256-byte bank row) lane (row r, quarter q) reads
//    slot (10 r + q + 4 step) mod 16: 10 r mod 16 is {0, 10, 4, 14} for r = 0..3 and {8, 2, 12, 6} for r = 12..15 -- the eight even
//    slots -- and for r = 4..11 the eight even slots again, which the next quarter's + 1 makes the eight odd ones: 16 distinct slots,
//    no conflict, in either kind of group and at every step (the substituted lanes of step 2 read quarter & 1, the same picture).  A
//    pitch of 72 or 88 (+ 8 halves of pad, the 64 form's habit) is 2-way by the same count, 80 and 112 are free; 80 needs no pad.
constexpr int HEAD_DIM_80 = 80;
constexpr int PITCH_80 = 80;
constexpr int VEC_80 = HEAD_DIM_80 / 8;  // 16-byte vectors per row

template <bool BF>
__global__ __launch_bounds__(AT) void mha_fwd_h80_kernel(const unsigned short* __restrict__ qkv, unsigned short* __restrict__ out, int s,
                                                          int heads, int q_tiles, float scale_log2e) {
    __shared__ __attribute__((aligned(16))) unsigned short k_lds[KV_TILE * PITCH_80];       // [key][dim]
    __shared__ __attribute__((aligned(16))) unsigned short vt_lds[HEAD_DIM_80 * PITCH_80];  // [dim][key slot] (slots 64..79 unused)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, quarter = lane >> 4;
    const long bid = blockIdx.x;
    const int qt = (int)(bid % q_tiles);
    const long bh = bid / q_tiles;
    const int head = (int)(bh % heads);
    const long b = bh / heads;
    const long row_stride = 3L * heads * HEAD_DIM_80;  // halves between consecutive tokens of qkv
    const unsigned short* base = qkv + b * s * row_stride + (long)head * HEAD_DIM_80;
    const unsigned short* kbase = base + (long)heads * HEAD_DIM_80;
    const unsigned short* vbase = base + 2L * heads * HEAD_DIM_80;

    const v4u zero4 = {0u, 0u, 0u, 0u};
    const int query = qt * 64 + wave * 16 + r16;
    const bool pad_lane = quarter >= 2;  // dims 80..95 of step 2
    v4u qf[3];
#pragma unroll
    for (int st = 0; st < 3; ++st)
        qf[st] = query < s && !(st == 2 && pad_lane) ? *reinterpret_cast<const v4u*>(base + (long)query * row_stride + 32 * st + 8 * quarter)
                                                     : zero4;

    f32x4 o[5];
#pragma unroll
    for (int db = 0; db < 5; ++db) o[db] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m_run = -INFINITY, l_run = 0.0f;  // l_run: this lane's share of the row sum (its 16 keys per tile)

    for (int k0 = 0; k0 < s; k0 += KV_TILE) {
        // this thread's part of the tile: vectors tid, tid + 256 and (tid < 128) tid + 512 of the 640; vector i is row i / 10, dims 8 (i % 10) .. + 7
        v4u kreg[3], vreg[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = tid + AT * i, row = idx / VEC_80, c = idx - row * VEC_80, key = k0 + row;
            const long off = (long)key * row_stride + 8 * c;
            const bool real = idx < KV_TILE * VEC_80 && key < s;
            kreg[i] = real ? *reinterpret_cast<const v4u*>(kbase + off) : zero4;
            vreg[i] = real ? *reinterpret_cast<const v4u*>(vbase + off) : zero4;
        }
        __syncthreads();  // every wave has finished reading the previous tile
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int idx = tid + AT * i, row = idx / VEC_80, c = idx - row * VEC_80;
            if (idx < KV_TILE * VEC_80) {
                *reinterpret_cast<v4u*>(&k_lds[row * PITCH_80 + 8 * c]) = kreg[i];
                const int slot = key_slot(row);
                const unsigned w[4] = {vreg[i].x, vreg[i].y, vreg[i].z, vreg[i].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vt_lds[(8 * c + 2 * e) * PITCH_80 + slot] = (unsigned short)(w[e] & 0xffffu);
                    vt_lds[(8 * c + 2 * e + 1) * PITCH_80 + slot] = (unsigned short)(w[e] >> 16);
                }
            }
        }
        __syncthreads();

        // S^T = K Q^T: 4 key groups x 3 steps over the 80 (+ 16 zero) dims
        f32x4 sc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int st = 0; st < 3; ++st) {
                const int col = st == 2 ? 64 + 8 * (quarter & 1) : 32 * st + 8 * quarter;  // (always inside the row's 80 dims)
                v4u a = *reinterpret_cast<const v4u*>(&k_lds[(16 * kt + r16) * PITCH_80 + col]);
                if (st == 2 && pad_lane) a = zero4;
                acc = mma16<BF>(a, qf[st], acc);
            }
            sc[kt] = acc;
        }
        float t_max = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * kt + 4 * quarter + r;
                const float t = key < s ? sc[kt][r] * scale_log2e : -INFINITY;
                sc[kt][r] = t;
                t_max = fmaxf(t_max, t);
            }
        t_max = fmaxf(t_max, __shfl_xor(t_max, 16, 64));
        t_max = fmaxf(t_max, __shfl_xor(t_max, 32, 64));
        const float m_new = fmaxf(m_run, t_max);            // finite: the tile holds a real key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0
        m_run = m_new;
        float p_sum = 0.0f;
        unsigned short ph[4][4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(sc[kt][r] - m_new);
                p_sum += p;
                ph[kt][r] = f32_to_half<BF>(p);
            }
        l_run = l_run * alpha + p_sum;
#pragma unroll
        for (int db = 0; db < 5; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[db][r] *= alpha;

        // O^T += V^T P^T: k-step s2 takes key groups 2 s2 (elements 0..3) and 2 s2 + 1 (elements 4..7)
        v4u pf[2];
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            pf[s2].x = (unsigned)ph[2 * s2][0] | ((unsigned)ph[2 * s2][1] << 16);
            pf[s2].y = (unsigned)ph[2 * s2][2] | ((unsigned)ph[2 * s2][3] << 16);
            pf[s2].z = (unsigned)ph[2 * s2 + 1][0] | ((unsigned)ph[2 * s2 + 1][1] << 16);
            pf[s2].w = (unsigned)ph[2 * s2 + 1][2] | ((unsigned)ph[2 * s2 + 1][3] << 16);
        }
#pragma unroll
        for (int db = 0; db < 5; ++db)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const v4u a = *reinterpret_cast<const v4u*>(&vt_lds[(16 * db + r16) * PITCH_80 + 32 * s2 + 8 * quarter]);
                o[db] = mma16<BF>(a, pf[s2], o[db]);
            }
    }

    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    if (query < s) {
        unsigned short* op = out + ((long)b * s + query) * ((long)heads * HEAD_DIM_80) + (long)head * HEAD_DIM_80 + 4 * quarter;
#pragma unroll
        for (int db = 0; db < 5; ++db) {
            uint2 w;
            w.x = (unsigned)f32_to_half<BF>(o[db][0] / l_tot) | ((unsigned)f32_to_half<BF>(o[db][1] / l_tot) << 16);
            w.y = (unsigned)f32_to_half<BF>(o[db][2] / l_tot) | ((unsigned)f32_to_half<BF>(o[db][3] / l_tot) << 16);
            *reinterpret_cast<uint2*>(op + 16 * db) = w;
        }
    }
}

}  // namespace

extern "C" int tia_mha_fwd_h(const void* d_qkv, void* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale,
                             int32_t dtype, void* stream) {
    if (!d_qkv || !d_out || n <= 0 || s <= 0 || heads <= 0 || head_dim <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (!(scale > 0.0f) || !(scale < INFINITY)) return TIA_EINVAL;
    if (head_dim != HEAD_DIM && head_dim != HEAD_DIM_80) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_qkv) | reinterpret_cast<uintptr_t>(d_out)) & 15) return TIA_EINVAL;
    if (s > 0x7fffffffL - KV_TILE || heads > 0x7fffffffL / (3 * head_dim)) return TIA_ESIZE;
    const long q_tiles = (s + 63) / 64;
    if (n > 0x7fffffffL / heads || n * heads > 0x7fffffffL / q_tiles) return TIA_ESIZE;  // one grid dimension
    const long blocks = n * heads * q_tiles;
    const float scale_log2e = scale * 1.44269504088896340736f;
    const bool bf = dtype == TIA_DT_BF16;
    const auto kernel = head_dim == HEAD_DIM_80 ? (bf ? mha_fwd_h80_kernel<true> : mha_fwd_h80_kernel<false>)
                                                : (bf ? mha_fwd_h_kernel<true> : mha_fwd_h_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(AT), 0, (hipStream_t)stream, (const unsigned short*)d_qkv,
                       (unsigned short*)d_out, (int)s, (int)heads, (int)q_tiles, scale_log2e);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
