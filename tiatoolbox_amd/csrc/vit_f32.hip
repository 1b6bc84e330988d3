// The float32 route of the Vision Transformer graph (models/architecture/vit_fused.py, prepare(torch.float32, linear_dtype="bfloat16x3");
// DESIGN 4.37): float32 activations, residual stream and row arithmetic; every Linear on the split-bf16 GEMM (conv_ring_bf16x3.hip) or
// the float32 MFMA GEMM (conv_mfma.hip).  This file holds what that graph needs beside them:
//   mha_fwd_f32      : attention on v_mfma_f32_16x16x4_f32 (exact float32 products and sums), head_dim 64 and 80
//   gelu_rows_f32    : x = 0.5 x (1 + erf(x / sqrt 2)) in place
//   swiglu_rows_f32  : y[r, j] = silu(x[r, j]) * x[r, H + j]
//   vit_patchify_f32 : float32 NHWC images -> [n, g, k_pad] float32 token rows, (ky, kx, c) order, zeros from 3 p^2 on
//   vit_assemble_f32 : out[b] = cat(cls (+ pos[0]), reg, tok[b] + pos[has_cls ..]), float32 tokens
// The LayerNorm, the pooled norm and the classifier head of that graph are tia_add_layernorm_rows_f32 (no branch, float32 out),
// tia_vit_cls_mean_pool_f32 (no branch) and tia_linear_softmax_rows_f32.  16 bytes per lane and access, 64-bit element offsets, no
// atomics; nothing here rounds to a half type.
//
// ---- mha_fwd_f32 -------------------------------------------------------------------------------------------------------------------
//   out[b, i, h, :] = softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) @ v[b, :, h, :]
// on the qkv Linear's own output order [n, s, 3, heads, hd] float32, written as [n, s, heads * hd] float32.  The structure is
// mha_fwd_h_kernel's (vit_attention.hip): one workgroup = (image, head, 64 queries), each of its 4 waves owns 16 query rows, K and V come
// in 64-key tiles through LDS, the first product is the SWAPPED one, S^T = K Q^T, the softmax is the online one, and the second
// product O^T = V^T P^T takes the probabilities as its B operand straight from the accumulators.
//
// v_mfma_f32_16x16x4_f32: every lane supplies ONE float per operand -- A[row l & 15][k = l >> 4], B[k = l >> 4][column l & 15] -- and
// holds D[row 4 (l >> 4) + r][column l & 15] in register r.  With quarter = l >> 4 and r16 = l & 15:
//  * First product, A = K (row = key), B = Q^T (column = query).  k-step (j, e), j < hd / 16, e < 4, sums over the four dims
//        dim = 16 j + 4 quarter + e
//    (any assignment of dims to (step, quarter) is a valid dot product as long as both operands use it): a lane's Q values of the four
//    steps e of one j are 16 contiguous bytes of its query's row -- hd / 16 global loads of 16 bytes, kept in registers -- and its K
//    values one 16-byte LDS read of row 16 kt + r16.  A key group's steps go to EIGHT accumulators, one per (j & 1, e) -- a chain of
//    2 or 3 instructions, 8 to 12 float32 fmas (quarter 0..3 inside an instruction, then j) -- which are then added pairwise,
//    ((e0 + e1) + (e2 + e3)) of j even + the same of j odd: a score is summed in short chains, not one chain of hd fmas, which keeps
//    the rounding after a dominant term at a few units (a 64 / 80-term chain measured 3 x the CPU's error on such data), and the
//    instruction's 40-cycle dependent latency is hidden by the seven other chains.  The sum of key group kt is
//        sc[kt][r] = score(query r16, key 16 kt + 4 quarter + r)
//    exactly as in the half kernel: row maximum and row sum are 15 register operations and two lane exchanges.
//  * Second product, A = V^T (row = an output dim), B = P^T (column = query): the B operand of k-step (kt, r) is the register sc[kt][r]
//    itself, so that step sums over the four keys
//        key = 16 kt + 4 quarter + r          (quarter = the instruction's k index)
//    and a tile's 64 keys are added to O in the order kt = 0..3, r = 0..3, the four quarters of a step in the order the instruction
//    sums its k (0, 1, 2, 3: a float32 fma chain).  One element per lane means V needs no transposed image: it stays [key][dim] in
//    LDS and lane (r16, quarter) reads row `key` of it.  Which output dim an A row stands for is free as well; it is chosen so that the
//    read is 16 bytes: block db < 4 of row r16 is dim 4 r16 + db (one 16-byte read serves four MFMAs), and head_dim 80 adds block 4,
//    dim 64 + r16 (a 4-byte read).  O^T's accumulators then hold, for the lane's query r16,
//        o[db][r] = O[dim 4 (4 quarter + r) + db]   (db < 4)        o[4][r] = O[dim 64 + 4 quarter + r]
//    -- 16 contiguous floats (+ 4 for head_dim 80) of the output row: 16-byte stores, no exchange for the rescale or the final 1 / l.
//  * head_dim 80 is 20 k-steps of 4 in the first product and a fifth block in the second: no padding dims anywhere.
//
// LDS: K rows at a pitch of hd + 8 floats, V rows at hd floats.  ds_read_b128 banks are (byte address / 4) mod 64 and conflicts count
// inside four 16-lane groups that hold rows {0-3, 12-15} of one quarter and rows {4-11} of the next (vit_attention.hip).  In 16-byte
// slots (16 per bank row) the K read of lane (row r, quarter q) is slot (c r + q + 4 j) mod 16 with c = (hd + 8) / 4 mod 16 = 2 (64) or
// 6 (80): c r is the eight even slots for r in {0-3, 12-15} and again for r in {4-11}, which the next quarter's + 1 makes the odd ones:
// no conflict.  The V read of lane (r16, q) is slot (r16 + (hd / 4) (4 q + r + 16 kt)) mod 16 = r16 + const, as 4 (hd / 4) is a multiple of
// 16 for both sizes: 16 distinct slots in every group.
//
// Arithmetic: exact float32 products and float32 sums throughout.  The running maximum m is kept in RAW score units and
// p = exp2((score - m) * scale * log2 e): the difference of two close scores is exact, so the rounding of the scaled value is relative to
// the (small) distance from the maximum, not to the size of the score.  p stays an unrounded float32 value in both the row sum and the
// second product; only O / l is written.  Keys >= s are loaded as zeros and their scores set to -inf BEFORE the maximum:
// p = exp2(-inf) = 0 exactly, and since every tile the loop visits holds at least one real key (k0 < s) the new maximum is finite from
// the first tile on: m_old - m_new is -inf - finite there, never inf - inf.  Query rows >= s compute on zeros and are not stored.
#include "conv_device.hpp"
#include "half_rows.hpp"
#include "vit_attention_tile.hpp"  // (mha::check_args)
#include "wide_io.hpp"

namespace {

using namespace tia;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int AT = 256;      // threads: 4 waves x 16 query rows
constexpr int KV_TILE = 64;  // keys per LDS tile
constexpr int ET = 256;      // threads of the row passes

__device__ __forceinline__ f32x4 mma4(float a, float b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int HD>
__global__ __launch_bounds__(AT) void mha_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int s, int heads,
                                                         int q_tiles, float scale_log2e) {
    constexpr int NJ = HD / 16;                 // 16-byte vectors of Q per lane = first-product steps / 4
    constexpr int VEC = HD / 4;                 // 16-byte vectors per row
    constexpr int PK = HD + 8, PV = HD;         // LDS row pitches in floats (see above)
    constexpr int PER = KV_TILE * VEC / AT;     // vectors of a tile per thread and operand: 4 (64) or 5 (80), no remainder
    constexpr int NDB = HD == 80 ? 5 : 4;       // output blocks of 16 dims
    static_assert((HD == 64 || HD == 80) && KV_TILE * VEC % AT == 0, "head_dim 64 or 80");
    __shared__ __attribute__((aligned(16))) float k_lds[KV_TILE * PK];  // [key][dim]
    __shared__ __attribute__((aligned(16))) float v_lds[KV_TILE * PV];  // [key][dim]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, quarter = lane >> 4;
    const long bid = blockIdx.x;
    const int qt = (int)(bid % q_tiles);
    const long bh = bid / q_tiles;
    const int head = (int)(bh % heads);
    const long b = bh / heads;
    const long row_stride = 3L * heads * HD;  // floats between consecutive tokens of qkv
    const float* base = qkv + b * s * row_stride + (long)head * HD;
    const float* kbase = base + (long)heads * HD;
    const float* vbase = base + 2L * heads * HD;

    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const int query = qt * 64 + wave * 16 + r16;
    f32x4 qf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
        qf[j] = query < s ? *reinterpret_cast<const f32x4*>(base + (long)query * row_stride + 16 * j + 4 * quarter) : zero4;

    f32x4 o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) o[db] = zero4;
    float m_run = -INFINITY, l_run = 0.0f;  // m_run in raw score units; l_run: this lane's share of the row sum (its 16 keys per tile)

    for (int k0 = 0; k0 < s; k0 += KV_TILE) {
        // this thread's part of the tile: vectors tid + 256 i of the 64 VEC; vector idx is row idx / VEC, dims 4 (idx % VEC) .. + 3
        f32x4 kreg[PER], vreg[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int idx = tid + AT * i, row = idx / VEC, c = idx - row * VEC, key = k0 + row;
            const long off = (long)key * row_stride + 4 * c;
            kreg[i] = key < s ? *reinterpret_cast<const f32x4*>(kbase + off) : zero4;
            vreg[i] = key < s ? *reinterpret_cast<const f32x4*>(vbase + off) : zero4;
        }
        __syncthreads();  // every wave has finished reading the previous tile
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int idx = tid + AT * i, row = idx / VEC, c = idx - row * VEC;
            *reinterpret_cast<f32x4*>(&k_lds[row * PK + 4 * c]) = kreg[i];
            *reinterpret_cast<f32x4*>(&v_lds[row * PV + 4 * c]) = vreg[i];
        }
        __syncthreads();

        // S^T = K Q^T: 4 key groups x HD / 4 steps, each group on eight independent chains (j parity, e) that are added pairwise
        f32x4 sc[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            f32x4 acc[2][4];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c >> 2][c & 3] = zero4;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&k_lds[(16 * kt + r16) * PK + 16 * j + 4 * quarter]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j & 1][e] = mma4(a[e], qf[j][e], acc[j & 1][e]);
            }
            sc[kt] = ((acc[0][0] + acc[0][1]) + (acc[0][2] + acc[0][3])) + ((acc[1][0] + acc[1][1]) + (acc[1][2] + acc[1][3]));
        }
        float t_max = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * kt + 4 * quarter + r;
                const float t = key < s ? sc[kt][r] : -INFINITY;
                sc[kt][r] = t;
                t_max = fmaxf(t_max, t);
            }
        t_max = fmaxf(t_max, __shfl_xor(t_max, 16, 64));
        t_max = fmaxf(t_max, __shfl_xor(t_max, 32, 64));
        const float m_new = fmaxf(m_run, t_max);                                    // finite: the tile holds a real key
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2e);  // first tile: exp2(-inf) = 0
        m_run = m_new;
        float p_sum = 0.0f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f((sc[kt][r] - m_new) * scale_log2e);
                p_sum += p;
                sc[kt][r] = p;
            }
        l_run = l_run * alpha + p_sum;
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[db][r] *= alpha;

        // O^T += V^T P^T: k-step (kt, r) sums over keys 16 kt + 4 quarter + r
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vrow = &v_lds[(16 * kt + 4 * quarter + r) * PV];
                const f32x4 a = *reinterpret_cast<const f32x4*>(vrow + 4 * r16);
                const float p = sc[kt][r];
#pragma unroll
                for (int db = 0; db < 4; ++db) o[db] = mma4(a[db], p, o[db]);
                if constexpr (HD == 80) o[4] = mma4(vrow[64 + r16], p, o[4]);
            }
    }

    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    if (query < s) {
        float* op = out + ((long)b * s + query) * ((long)heads * HD) + (long)head * HD;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<f32x4*>(op + 16 * quarter + 4 * r) = f32x4{o[0][r] / l_tot, o[1][r] / l_tot, o[2][r] / l_tot, o[3][r] / l_tot};
        if constexpr (HD == 80)
            *reinterpret_cast<f32x4*>(op + 64 + 4 * quarter) = f32x4{o[4][0] / l_tot, o[4][1] / l_tot, o[4][2] / l_tot, o[4][3] / l_tot};
    }
}

// ---- the row passes: one thread per 4 floats (16 bytes) ---------------------------------------------------------------------------------

// Exact (erf) GELU.  For x >= 0 it is torch's expression 0.5 x (1 + erf(x / sqrt 2)); for x < 0 the same value is written as
// 0.5 x erfc(-x / sqrt 2), which has no 1 - 0.99999... cancellation in the tail.  -0.0 stays -0.0 (0.5 * -0 * 1).
__device__ __forceinline__ float gelu_f32(float x) {
    const float t = x * 0.70710678118654752440f;
    return x >= 0.0f ? 0.5f * x * (1.0f + erff(t)) : 0.5f * x * erfcf(-t);
}

__global__ __launch_bounds__(ET) void gelu_rows_f32_kernel(f32x4* __restrict__ x, long vectors) {
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        f32x4 v = x[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = gelu_f32(v[k]);
        x[i] = v;
    }
}

// the gate vector at [r, 4 j] and the value vector at [r, H + 4 j] (H % 4 == 0 makes every row and its second half start on a vector)
__global__ __launch_bounds__(ET) void swiglu_rows_f32_kernel(const f32x4* __restrict__ x, long vectors, int hv, f32x4* __restrict__ y) {
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const long r = i / hv;
        const int j = (int)(i - r * hv);
        const f32x4 gate = x[r * (2L * hv) + j], val = x[r * (2L * hv) + hv + j];
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = silu_f32(gate[k]) * val[k];
        y[i] = v;
    }
}

// vit_patchify_pad_h_kernel's gather on float32: a patch row (3 p values) starts on no 16-byte boundary in the image in general, so
// the 4 values are read one by one (aligned 4-byte loads; neighbouring lanes read neighbouring addresses) while (ky, position in the
// run) steps along; columns from 3 p^2 on are zeros.  One aligned 16-byte store (k_pad % 4 == 0).
__global__ __launch_bounds__(ET) void vit_patchify_f32_kernel(const float* __restrict__ x, int h, int w, int p, int kv, long vectors,
                                                              f32x4* __restrict__ out) {
    const int run = 3 * p, k_real = run * p, gw = w / p, gh = h / p;
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const int v = (int)(i % kv);
        long t = i / kv;
        const int gx = (int)(t % gw);
        t /= gw;
        const int gy = (int)(t % gh);
        const long b = t / gh;
        int k = 4 * v, ky = k / run, rem = k - ky * run;
        const long base = ((b * h + (long)gy * p) * w + (long)gx * p) * 3;  // the patch's first value; a row further down is + 3 w
        f32x4 f;
#pragma unroll
        for (int e = 0; e < 4; ++e, ++k) {
            if (k < k_real) {
                f[e] = x[base + (long)ky * w * 3 + rem];
                if (++rem == run) rem = 0, ++ky;
            } else {
                f[e] = 0.0f;
            }
        }
        out[i] = f;
    }
}

// vit_assemble_rows_f32_kernel (vit_rows.hip) for float32 tokens: the same rows, the same single float32 add.
__global__ __launch_bounds__(ET) void vit_assemble_f32_kernel(const f32x4* __restrict__ tok, const f32x4* __restrict__ cls,
                                                              const f32x4* __restrict__ reg, const f32x4* __restrict__ pos, int has_cls,
                                                              long vectors, int g, int nreg, int dv, f32x4* __restrict__ out) {
    const int s = 1 + nreg + g;
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const int v = (int)(i % dv);
        const long t = i / dv;
        const int tk = (int)(t % s);
        const long b = t / s;
        f32x4 a;
        long prow = -1;  // the row of `pos` to add, if any
        if (tk == 0) {
            a = cls[v];
            if (has_cls) prow = 0;
        } else if (tk <= nreg) {
            a = reg[(long)(tk - 1) * dv + v];
        } else {
            const int pi = tk - 1 - nreg;
            a = tok[(b * g + pi) * dv + v];
            prow = pi + has_cls;
        }
        if (prow >= 0) a += pos[prow * dv + v];
        out[i] = a;
    }
}

unsigned stream_blocks(long items) {
    long blocks = (items + ET - 1) / ET;
    if (blocks > 256L * 64) blocks = 256L * 64;
    return (unsigned)blocks;
}

}  // namespace

extern "C" int tia_mha_fwd_f32(const float* d_qkv, float* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale,
                               int32_t dtype, void* stream) {
    long q_tiles;
    const int code = mha::check_args(d_qkv, d_out, n, s, heads, head_dim, scale, dtype == TIA_DT_F32, s, heads, &q_tiles);
    if (code != TIA_OK) return code;
    const long blocks = n * heads * q_tiles;
    const float scale_log2e = scale * 1.44269504088896340736f;
    const auto kernel = head_dim == 80 ? mha_fwd_f32_kernel<80> : mha_fwd_f32_kernel<64>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(AT), 0, (hipStream_t)stream, d_qkv, d_out, (int)s, (int)heads, (int)q_tiles,
                       scale_log2e);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_gelu_rows_f32(float* d_x, int64_t count, void* stream) {
    if (!d_x || count <= 0) return TIA_EINVAL;
    if ((count & 3) != 0) return TIA_ESIZE;
    if (reinterpret_cast<uintptr_t>(d_x) & 15) return TIA_EINVAL;
    const long vectors = count / 4;
    hipLaunchKernelGGL(gelu_rows_f32_kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, (f32x4*)d_x, vectors);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_swiglu_rows_f32(const float* d_x, float* d_y, int64_t rows, int64_t hidden, void* stream) {
    if (!d_x || !d_y || rows <= 0 || hidden <= 0) return TIA_EINVAL;
    if ((hidden & 3) != 0 || hidden > 0x3fffffffL || rows > 0x7fffffffL) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y)) & 15) return TIA_EINVAL;
    const long vectors = rows * (hidden / 4);
    hipLaunchKernelGGL(swiglu_rows_f32_kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, (const f32x4*)d_x, vectors,
                       (int)(hidden / 4), (f32x4*)d_y);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_patchify_f32(const float* d_x, float* d_tokens, int64_t n, int64_t h, int64_t w, int64_t patch, int64_t k_pad,
                                    void* stream) {
    if (!d_x || !d_tokens || n <= 0 || h <= 0 || w <= 0 || patch <= 0 || k_pad <= 0) return TIA_EINVAL;
    if (h % patch != 0 || w % patch != 0) return TIA_ESIZE;
    if (h > 0x7fffffffL / 3 || w > 0x7fffffffL / 3 || n > 0x7fffffffL || patch > 16384) return TIA_ESIZE;  // (3 p^2 stays an int)
    if ((k_pad & 15) != 0 || k_pad < 3 * patch * patch || k_pad > 0x7ffffff0L) return TIA_ESIZE;
    // the image is read with 4-byte loads (a batch may be a slice that starts at any float of a larger buffer); the rows are stored 16 bytes wide
    if ((reinterpret_cast<uintptr_t>(d_x) & 3) != 0 || (reinterpret_cast<uintptr_t>(d_tokens) & 15) != 0) return TIA_EINVAL;
    const long vectors = n * (h / patch) * (w / patch) * (k_pad / 4);
    hipLaunchKernelGGL(vit_patchify_f32_kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, d_x, (int)h, (int)w,
                       (int)patch, (int)(k_pad / 4), vectors, (f32x4*)d_tokens);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_assemble_f32(const float* d_tokens, const float* d_cls, const float* d_reg, const float* d_pos, int32_t pos_has_cls,
                                    float* d_out, int64_t n, int64_t g, int64_t reg_tokens, int64_t d, void* stream) {
    if (!d_tokens || !d_cls || !d_pos || !d_out || n <= 0 || g <= 0 || d <= 0 || reg_tokens < 0) return TIA_EINVAL;
    if ((reg_tokens > 0) != (d_reg != nullptr) || (pos_has_cls != 0 && pos_has_cls != 1)) return TIA_EINVAL;
    if ((d & 3) != 0 || d > 8192) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_tokens) | reinterpret_cast<uintptr_t>(d_cls) | reinterpret_cast<uintptr_t>(d_reg) |
         reinterpret_cast<uintptr_t>(d_pos) | reinterpret_cast<uintptr_t>(d_out)) & 15)
        return TIA_EINVAL;
    if (g > 0x3fffffffL || reg_tokens > 0x3fffffffL || n > 0x7fffffffL) return TIA_ESIZE;
    const long vectors = n * (1 + reg_tokens + g) * (d / 4);
    hipLaunchKernelGGL(vit_assemble_f32_kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, (const f32x4*)d_tokens,
                       (const f32x4*)d_cls, (const f32x4*)d_reg, (const f32x4*)d_pos, (int)pos_has_cls, vectors, (int)g, (int)reg_tokens,
                       (int)(d / 4), (f32x4*)d_out);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
