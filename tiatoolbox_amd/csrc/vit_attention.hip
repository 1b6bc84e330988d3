// Fused multi-head attention forward for the Vision Transformers (fp16 / bf16; head_dim 64 and 80 are ONE kernel, mha_fwd_h_kernel<BF, HD>),
// on v_mfma_f32_16x16x32_f16 / _bf16:
//   out[b, i, h, :] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) @ v[b, :, h, :]
// on the qkv Linear's own output order [n, s, 3, heads, hd] (no permute pass), written as [n, s, heads * hd].
//
// One workgroup = (image, head, 64 queries); each of its 4 waves owns 16 query rows, whose Q stays in registers as the B operand
// (lane l: query l & 15, dims 32 step + 8 (l >> 4) .. + 7: one 16-byte global load per step).  K and V come in 64-key tiles through
// LDS.  The first product is the SWAPPED one, S^T = K Q^T: A = K (row = key), so the accumulator of key group kt holds
//   sc[kt][r] = score(query l & 15, key 16 kt + 4 (l >> 4) + r)
// -- a query's 64 scores of a tile sit in the 16 registers of the four lanes l & 15, l & 15 + 16, + 32, + 48.  Row maximum and row sum are
// 15 register operations and two lane exchanges; the running maximum m and the sum l live in the lane of their query.
// The second product is O^T = V^T P^T with B = P^T: the rounded accumulators ARE that operand, with no lane movement and no LDS:
// element j of lane quarter q in k-step s2 is key 32 s2 + 16 (j >> 2) + 4 q + (j & 3).  V is therefore written to LDS transposed
// ([dim][key]) with the keys of a row in exactly that order (key_slot), so that the A operand (row = dim 16 db + (l & 15))
// is one 16-byte LDS read.  O^T's accumulator has the query on the lane again (o[db][r] = O[query l & 15][dim 16 db + 4 (l >> 4) + r]),
// so the rescale by exp2(m_old - m_new) and the final 1 / l need no exchange either.
//
// Arithmetic: float32 online softmax in the base-2 domain (t = dot * scale * log2 e); the sum is taken over the unrounded float32 p, p is
// rounded once to the half type for the MFMA, the output O / l is rounded once.  Keys >= s are loaded as zeros and their scores set
// to -inf BEFORE the maximum: p = exp2(-inf - m) = 0 exactly, and since every tile the loop visits holds at least one real key
// (k0 < s) the new maximum is finite from the first tile on: m_old - m_new is -inf - finite there, never inf - inf.  Query rows >= s
// compute on zeros and are not stored.
//
// The tile geometry per head_dim, the workgroup decode, the Q load, the staging, the score tile and the online maximum are
// vit_attention_tile.hpp's, which the probabilities kernel (vit_attention_maps.hip) is built from as well.
#include "vit_attention_tile.hpp"

namespace {

using namespace tia;
using namespace tia::mha;

template <bool BF, int HD>
__global__ __launch_bounds__(AT) void mha_fwd_h_kernel(const unsigned short* __restrict__ qkv, unsigned short* __restrict__ out, int s,
                                                        int heads, int q_tiles, float scale_log2e) {
    using G = Geo<HD>;
    __shared__ __attribute__((aligned(16))) unsigned short k_lds[KV_TILE * G::PITCH];  // [key][dim]
    __shared__ __attribute__((aligned(16))) unsigned short vt_lds[HD * G::PITCH];      // [dim][key slot]

    const Where w = decode(q_tiles);  // rest = (image, head)
    const int r16 = w.r16, quarter = w.quarter, query = w.query;
    const int head = (int)(w.rest % heads);
    const long b = w.rest / heads;
    const long row_stride = 3L * heads * HD;  // halves between consecutive tokens of qkv
    const unsigned short* base = qkv + b * s * row_stride + (long)head * HD;
    const unsigned short* kbase = base + (long)heads * HD;
    const unsigned short* vbase = base + 2L * heads * HD;

    v4u qf[G::STEPS];
    load_q<HD>(base, row_stride, query, s, quarter, qf);

    f32x4 o[G::BLOCKS];
#pragma unroll
    for (int db = 0; db < G::BLOCKS; ++db) o[db] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m_run = -INFINITY, l_run = 0.0f;

    for (int k0 = 0; k0 < s; k0 += KV_TILE) {
        stage_tile<HD, true>(kbase, vbase, row_stride, k0, s, w.tid, k_lds, vt_lds);
        f32x4 t[4];
        const float t_max = score_tile<BF, HD>(k_lds, qf, k0, s, r16, quarter, scale_log2e, t);
        unsigned short ph[4][4];  // p rounded once, for the second product
        const float alpha = online_max(t_max, m_run);
        float p_sum = 0.0f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(t[kt][r] - m_run);
                p_sum += p;
                ph[kt][r] = f32_to_half<BF>(p);
            }
        l_run = l_run * alpha + p_sum;
#pragma unroll
        for (int db = 0; db < G::BLOCKS; ++db)
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
        for (int db = 0; db < G::BLOCKS; ++db)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const v4u a = *reinterpret_cast<const v4u*>(&vt_lds[(16 * db + r16) * G::PITCH + 32 * s2 + 8 * quarter]);
                o[db] = mma16<BF>(a, pf[s2], o[db]);
            }
    }

    const float l_tot = row_sum(l_run);
    if (query < s) {
        unsigned short* op = out + ((long)b * s + query) * ((long)heads * HD) + (long)head * HD + 4 * quarter;
#pragma unroll
        for (int db = 0; db < G::BLOCKS; ++db) {
            uint2 w2;
            w2.x = (unsigned)f32_to_half<BF>(o[db][0] / l_tot) | ((unsigned)f32_to_half<BF>(o[db][1] / l_tot) << 16);
            w2.y = (unsigned)f32_to_half<BF>(o[db][2] / l_tot) | ((unsigned)f32_to_half<BF>(o[db][3] / l_tot) << 16);
            *reinterpret_cast<uint2*>(op + 16 * db) = w2;
        }
    }
}

}  // namespace

extern "C" int tia_mha_fwd_h(const void* d_qkv, void* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale,
                             int32_t dtype, void* stream) {
    long q_tiles;
    const int code = check_args(d_qkv, d_out, n, s, heads, head_dim, scale, dtype == TIA_DT_F16 || dtype == TIA_DT_BF16, s, heads, &q_tiles);
    if (code != TIA_OK) return code;
    const long blocks = n * heads * q_tiles;
    const float scale_log2e = scale * 1.44269504088896340736f;
    const bool bf = dtype == TIA_DT_BF16;
    const auto kernel = head_dim == 80 ? (bf ? mha_fwd_h_kernel<true, 80> : mha_fwd_h_kernel<false, 80>)
                                       : (bf ? mha_fwd_h_kernel<true, 64> : mha_fwd_h_kernel<false, 64>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(AT), 0, (hipStream_t)stream, (const unsigned short*)d_qkv,
                       (unsigned short*)d_out, (int)s, (int)heads, (int)q_tiles, scale_log2e);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
