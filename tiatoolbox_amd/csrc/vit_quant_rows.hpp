// The Vision Transformer linear layers on an 8-bit matrix instruction, once for every number format (vit_fp8.hip: E4m3, vit_int8.hip:
// Int8): the GEMM on row x column scaled codes, the weight packer, the quantising LayerNorm and GELU / SwiGLU producers,
// and their launchers.  A format F is a struct with
//   code_t                    the byte type of a code
//   acc_t, zero()             the accumulator vector of one 16 x 16 tile and its zero
//   step(w, t, acc)           the matrix instruction(s) of one 128-deep K-step on one tile; an operand is a lane's 32 bytes (v8i),
//                             which an instruction that takes 16 splits into its two pieces
//   amax(a, b)                the larger of two magnitudes (what a NaN does is the format's)
//   row_scales(amax, inv, s)  (inv, s) of a row with largest magnitude amax
//   code(x)                   float32 -> one code, as the low byte of an unsigned
//   K_MAX                     the largest K the accumulator takes
// and everything below is written against that.  The kernels and launchers have internal linkage: each of the two files instantiates
// them for its own format.
#pragma once
#include <type_traits>

#include "half_rows.hpp"

namespace tia::q8 {

using v2u = __attribute__((ext_vector_type(2))) unsigned;
using v8i = __attribute__((ext_vector_type(8))) int;

constexpr int ET = 256;

namespace {

// ---- the GEMM -------------------------------------------------------------------------------------------------------------------
// A workgroup of four waves makes a tile of 128 output channels x 128 tokens; a wave a quarter of 64 x 64 as 4 x 4 MFMA tiles.  The
// WEIGHTS are the instruction's A operand and the tokens its B operand: D then has the token on the lane (lane & 15) and four
// CONSECUTIVE channels (4 (lane >> 4) + register) in a lane's four registers, which the epilogue stores as one 8-byte vector.
// Both operands are [row][K] bytes in memory and are staged alike: per 128-deep K-step 128 rows x 128 bytes each, fetched as 16-byte
// pieces into registers one step ahead (in flight during the step's MFMAs) and written to an LDS image of 8 pieces per row with
// the piece index XORed with row & 7.  A lane's fragment is the 32 bytes k = 32 (lane >> 4) .. + 31 of row lane & 15 (pieces
// 2 (lane >> 4) and 2 (lane >> 4) + 1) for BOTH operands: the sum over k pairs byte j of A's lane with byte j of B's lane, so the
// result does not depend on which k the hardware assigns to a byte as long as it does so alike for A and B (the exact tests are the
// check of that).
// Rows beyond the operand's end are read from its last row (in range, never stored): a row of a GEMM only reaches its own outputs.
constexpr int BT = 128;         // tile side, both ways
constexpr int PIECES = BT * 8;  // 16-byte pieces of one operand's K-step

template <class F, bool BF>
__global__ __launch_bounds__(ET) void linear_rows_kernel(const typename F::code_t* __restrict__ a, const float* __restrict__ sa,
                                                          const typename F::code_t* __restrict__ w, const float* __restrict__ sw,
                                                          const float* __restrict__ bias, const unsigned short* __restrict__ res,
                                                          unsigned short* __restrict__ y, long rows, int n, int k, int n_ct) {
    using code_t = typename F::code_t;
    __shared__ v4u lds[2 * PIECES];  // [0, PIECES): weights, [PIECES, 2 PIECES): tokens
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)(blockIdx.x % n_ct) * BT;
    const long t0 = (long)(blockIdx.x / n_ct) * BT;

    // staging: thread t carries piece t & 7 of rows (t >> 3) + 32 i, i = 0 .. 3, of each operand
    const int srow = tid >> 3, piece = tid & 7;
    const code_t* wsrc[4];
    const code_t* asrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int wr = min(c0 + srow + 32 * i, n - 1);
        const long ar = min(t0 + srow + 32 * i, rows - 1);
        wsrc[i] = w + (long)wr * k + 16 * piece;
        asrc[i] = a + ar * k + 16 * piece;
    }
    const int sdst = srow * 8 + (piece ^ (srow & 7));
    v4u wreg[4], areg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        wreg[i] = *reinterpret_cast<const v4u*>(wsrc[i]);
        areg[i] = *reinterpret_cast<const v4u*>(asrc[i]);
    }

    const int r = lane & 15, g = lane >> 4;
    const int wm = wave & 1, wt = wave >> 1;
    const int p0 = (2 * g) ^ (r & 7), p1 = (2 * g + 1) ^ (r & 7);
    typename F::acc_t acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) acc[mi][ti] = F::zero();

    const int steps = k / 128;
    for (int kt = 0; kt < steps; ++kt) {
        __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lds[sdst + 256 * i] = wreg[i];
            lds[PIECES + sdst + 256 * i] = areg[i];
        }
        __syncthreads();
        if (kt + 1 < steps) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                wreg[i] = *reinterpret_cast<const v4u*>(wsrc[i] + 128L * (kt + 1));
                areg[i] = *reinterpret_cast<const v4u*>(asrc[i] + 128L * (kt + 1));
            }
        }
        v8i tf[4];
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
            const int row = wt * 64 + ti * 16 + r;
            const v4u lo = lds[PIECES + row * 8 + p0], hi = lds[PIECES + row * 8 + p1];
            tf[ti] = v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = wm * 64 + mi * 16 + r;
            const v4u lo = lds[row * 8 + p0], hi = lds[row * 8 + p1];
            const v8i wf = v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) acc[mi][ti] = F::step(wf, tf[ti], acc[mi][ti]);
        }
    }

    // epilogue: lane = token (r) x four consecutive channels (4 g ..); n % 16 == 0 keeps a lane's four channels on one side of n
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const long tok = t0 + wt * 64 + ti * 16 + r;
        if (tok >= rows) continue;
        const float s_tok = sa[tok];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int ch = c0 + wm * 64 + mi * 16 + 4 * g;
            if (ch >= n) continue;
            const float4 s_ch = *reinterpret_cast<const float4*>(sw + ch);
            float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (bias) b = *reinterpret_cast<const float4*>(bias + ch);
            float o[4] = {(float)acc[mi][ti][0] * s_tok * s_ch.x + b.x, (float)acc[mi][ti][1] * s_tok * s_ch.y + b.y,
                          (float)acc[mi][ti][2] * s_tok * s_ch.z + b.z, (float)acc[mi][ti][3] * s_tok * s_ch.w + b.w};
            const long at = tok * n + ch;
            if (res) {
                const v2u rv = *reinterpret_cast<const v2u*>(res + at);
                o[0] += half_to_f32<BF>((unsigned short)(rv.x & 0xffffu));
                o[1] += half_to_f32<BF>((unsigned short)(rv.x >> 16));
                o[2] += half_to_f32<BF>((unsigned short)(rv.y & 0xffffu));
                o[3] += half_to_f32<BF>((unsigned short)(rv.y >> 16));
            }
            v2u ov;
            ov.x = (unsigned)f32_to_half<BF>(o[0]) | ((unsigned)f32_to_half<BF>(o[1]) << 16);
            ov.y = (unsigned)f32_to_half<BF>(o[2]) | ((unsigned)f32_to_half<BF>(o[3]) << 16);
            *reinterpret_cast<v2u*>(y + at) = ov;
        }
    }
}

// ---- quantising one row ---------------------------------------------------------------------------------------------------------

template <class F>
__device__ __forceinline__ float wave_amax(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = F::amax(v, __shfl_xor(v, m, 64));
    return v;
}

template <class F>
__device__ __forceinline__ v2u codes8(const float (&f)[8], float inv) {
    unsigned c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = F::code(f[j] * inv);
    v2u o;
    o.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    o.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
    return o;
}

// The row's float32 values are in f (this lane's vectors lane + 64 i, below cv): the row maximum over the wave, then the codes as
// one 8-byte store per vector and the scale from lane 0.
template <class F, int VPL>
__device__ __forceinline__ void quantise_row(const float (&f)[VPL][8], int lane, int cv, typename F::code_t* qrow, float* srow) {
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = F::amax(amax, fabsf(f[i][j]));
        }
    amax = wave_amax<F>(amax);
    float inv, s;
    F::row_scales(amax, inv, s);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) *reinterpret_cast<v2u*>(qrow + 8 * v) = codes8<F>(f[i], inv);
    }
    if (lane == 0) *srow = s;
}

// The float32 values of one LayerNorm row in a wave's registers (layernorm_rows_h_kernel's form and arithmetic: the mean, then the
// variance of the centred values, the affine as one fmaf): f holds this lane's vectors lane + 64 i, below cv = c / 8.
template <bool BF, int VPL>
__device__ __forceinline__ void layernorm_row_values(const unsigned short* __restrict__ xr, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, int c, int lane, float (&f)[VPL][8]) {
    const int cv = c >> 3;
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            unpack8<BF>(*reinterpret_cast<const v4u*>(xr + 8 * v), f[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += f[i][j];
        }
    }
    const float mean = wave_sum(sum) / (float)c;
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                f[i][j] -= mean;
                sq = fmaf(f[i][j], f[i][j], sq);
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)c + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            float gm[8], bt[8];
            load8_f32(gamma + 8 * v, gm);
            load8_f32(beta + 8 * v, bt);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[i][j] = fmaf(f[i][j] * rstd, gm[j], bt[j]);
        }
    }
}

// One wave per row, the row in registers, four rows per workgroup; what layernorm_rows_h_kernel would round to half is quantised here.
template <class F, bool BF, int VPL>
__global__ __launch_bounds__(ET) void layernorm_rows_kernel(const unsigned short* __restrict__ x, long stride, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps, long rows, int c,
                                                             typename F::code_t* __restrict__ q, float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;  // whole waves leave: the exchanges below stay inside a wave
    float f[VPL][8];
    layernorm_row_values<BF, VPL>(x + row * stride, gamma, beta, eps, c, lane, f);
    quantise_row<F, VPL>(f, lane, c >> 3, q + row * (long)c, s + row);
}

// The float32 values of the activation between fc1 and fc2 for one row of `hidden` outputs.  SWIGLU: the input row is
// [gate H | value H].
template <bool BF, bool SWIGLU, int VPL>
__device__ __forceinline__ void act_row_values(const unsigned short* __restrict__ xr, int hidden, int lane, float (&f)[VPL][8]) {
    const int cv = hidden >> 3;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            unpack8<BF>(*reinterpret_cast<const v4u*>(xr + 8 * v), f[i]);
            if constexpr (SWIGLU) {
                float val[8];
                unpack8<BF>(*reinterpret_cast<const v4u*>(xr + hidden + 8 * v), val);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[i][j] = silu_f32(f[i][j]) * val[j];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) f[i][j] = 0.5f * f[i][j] * (1.0f + erff(f[i][j] * 0.70710678118654752440f));
            }
        }
    }
}

// The activation, one wave per row, quantised.
template <class F, bool BF, bool SWIGLU, int VPL>
__global__ __launch_bounds__(ET) void act_rows_kernel(const unsigned short* __restrict__ x, long rows, int hidden,
                                                       typename F::code_t* __restrict__ q, float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    float f[VPL][8];
    act_row_values<BF, SWIGLU, VPL>(x + row * (SWIGLU ? 2L : 1L) * hidden, hidden, lane, f);
    quantise_row<F, VPL>(f, lane, hidden >> 3, q + row * (long)hidden, s + row);
}

// The same with per-input-channel smoothing: every float32 value is multiplied by inv_smooth[channel] -- one float32
// multiplication, exact for the power-of-two scales the graph makes -- before the row maximum and the codes.
template <class F, bool BF, bool SWIGLU, int VPL>
__global__ __launch_bounds__(ET) void act_rows_smooth_kernel(const unsigned short* __restrict__ x, const float* __restrict__ inv_smooth,
                                                              long rows, int hidden, typename F::code_t* __restrict__ q,
                                                              float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int cv = hidden >> 3;
    float f[VPL][8];
    act_row_values<BF, SWIGLU, VPL>(x + row * (SWIGLU ? 2L : 1L) * hidden, hidden, lane, f);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            float sm[8];
            load8_f32(inv_smooth + 8 * v, sm);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[i][j] *= sm[j];
        }
    }
    quantise_row<F, VPL>(f, lane, cv, q + row * (long)hidden, s + row);
}

// Weights: one wave per output channel, the row read twice (the maximum, then the codes; the second read is served by the cache --
// this runs once per layer, in `prepare`).  k % 4 == 0.
template <class F>
__global__ __launch_bounds__(ET) void pack_weights_kernel(const float* __restrict__ w, long n, int k, typename F::code_t* __restrict__ q,
                                                           float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const float4* wr = reinterpret_cast<const float4*>(w + row * (long)k);
    float amax = 0.0f;
    for (int v = lane; v < k / 4; v += 64) {
        const float4 t = wr[v];
        amax = F::amax(F::amax(amax, F::amax(fabsf(t.x), fabsf(t.y))), F::amax(fabsf(t.z), fabsf(t.w)));
    }
    amax = wave_amax<F>(amax);
    float inv, sc;
    F::row_scales(amax, inv, sc);
    unsigned* qr = reinterpret_cast<unsigned*>(q + row * (long)k);
    for (int v = lane; v < k / 4; v += 64) {
        const float4 t = wr[v];
        qr[v] = F::code(t.x * inv) | (F::code(t.y * inv) << 8) | (F::code(t.z * inv) << 16) | (F::code(t.w * inv) << 24);
    }
    if (lane == 0) s[row] = sc;
}

// ---- the host side --------------------------------------------------------------------------------------------------------------

inline bool misaligned(std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15) != 0;
}

inline bool is_half(int32_t dtype) { return dtype == TIA_DT_F16 || dtype == TIA_DT_BF16; }

inline int launched() { return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH; }

// the shapes the GEMM takes: 0, or the error code of everything else
template <class F>
int linear_shape(int64_t rows, int64_t n, int64_t k) {
    if (rows <= 0 || n <= 0 || k <= 0) return TIA_EINVAL;
    if (k % 128 != 0 || n % 16 != 0 || k > F::K_MAX || n > (1 << 24)) return TIA_ESIZE;
    const int64_t tiles = ((rows + BT - 1) / BT) * ((n + BT - 1) / BT);
    if (rows > (int64_t(1) << 40) || tiles > 0x7fffffffL) return TIA_ESIZE;
    return TIA_OK;
}

template <class F>
int serves(int64_t rows, int64_t n, int64_t k) {
    const int rc = linear_shape<F>(rows, n, k);
    return rc == TIA_OK ? 1 : (rc == TIA_ESIZE ? 0 : rc);
}

template <class F>
int linear_rows(const void* d_a, const float* d_sa, const void* d_w, const float* d_sw, const float* d_bias, const void* d_residual,
                void* d_y, int64_t rows, int64_t n, int64_t k, int32_t dtype, void* stream) {
    using code_t = typename F::code_t;
    if (!d_a || !d_sa || !d_w || !d_sw || !d_y) return TIA_EINVAL;
    if (!is_half(dtype)) return TIA_EINVAL;
    const int rc = linear_shape<F>(rows, n, k);
    if (rc != TIA_OK) return rc;
    if (misaligned({d_a, d_sa, d_w, d_sw, d_bias, d_residual, d_y})) return TIA_EINVAL;
    const int n_ct = (int)((n + BT - 1) / BT);
    const dim3 grid((unsigned)(((rows + BT - 1) / BT) * n_ct));
    const auto kernel = dtype == TIA_DT_BF16 ? linear_rows_kernel<F, true> : linear_rows_kernel<F, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(ET), 0, (hipStream_t)stream, static_cast<const code_t*>(d_a), d_sa,
                       static_cast<const code_t*>(d_w), d_sw, d_bias, static_cast<const unsigned short*>(d_residual),
                       static_cast<unsigned short*>(d_y), (long)rows, (int)n, (int)k, n_ct);
    return launched();
}

template <class F>
int pack_weights(const float* d_w, int64_t n, int64_t k, void* d_q, float* d_scale, void* stream) {
    if (!d_w || !d_q || !d_scale) return TIA_EINVAL;
    const int rc = linear_shape<F>(1, n, k);
    if (rc != TIA_OK) return rc;
    if (misaligned({d_w, d_q, d_scale})) return TIA_EINVAL;
    const dim3 grid((unsigned)((n + ET / 64 - 1) / (ET / 64)));
    hipLaunchKernelGGL(pack_weights_kernel<F>, grid, dim3(ET), 0, (hipStream_t)stream, d_w, (long)n, (int)k,
                       static_cast<typename F::code_t*>(d_q), d_scale);
    return launched();
}

// The producers hold a row of c values in a wave's registers, VPL = 1, 2, 4, 8 or 16 vectors of 8 per lane: launch(BF, VPL), both as
// integral constants, for the half type of `dtype` and the smallest VPL that holds the row.
template <class Launch>
void for_row_width(int32_t dtype, int64_t c, Launch launch) {
    const int vpl = (int)((c / 8 + 63) / 64);
    const auto by_vpl = [&](auto bf) {
        if (vpl <= 1) launch(bf, std::integral_constant<int, 1>{});
        else if (vpl <= 2) launch(bf, std::integral_constant<int, 2>{});
        else if (vpl <= 4) launch(bf, std::integral_constant<int, 4>{});
        else if (vpl <= 8) launch(bf, std::integral_constant<int, 8>{});
        else launch(bf, std::integral_constant<int, 16>{});
    };
    if (dtype == TIA_DT_BF16) by_vpl(std::true_type{});
    else by_vpl(std::false_type{});
}

template <class F>
int layernorm_rows(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, void* d_q, float* d_scale,
                   int64_t rows, int64_t c, int32_t dtype, void* stream) {
    if (!d_x || !d_gamma || !d_beta || !d_q || !d_scale || rows <= 0 || c <= 0 || !(eps >= 0.0f)) return TIA_EINVAL;
    if (!is_half(dtype)) return TIA_EINVAL;
    if ((c & 15) != 0 || c > 8192) return TIA_ESIZE;
    if (row_stride < c || (row_stride & 7) != 0) return TIA_EINVAL;
    if (misaligned({d_x, d_gamma, d_beta, d_q, d_scale})) return TIA_EINVAL;
    const long blocks = (rows + ET / 64 - 1) / (ET / 64);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    for_row_width(dtype, c, [&](auto bf, auto vpl) {
        hipLaunchKernelGGL((layernorm_rows_kernel<F, decltype(bf)::value, decltype(vpl)::value>), dim3((unsigned)blocks), dim3(ET), 0, (hipStream_t)stream,
                           static_cast<const unsigned short*>(d_x), (long)row_stride, d_gamma, d_beta, eps, (long)rows, (int)c,
                           static_cast<typename F::code_t*>(d_q), d_scale);
    });
    return launched();
}

template <class F, bool SWIGLU>
int act_rows(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    if (!d_x || !d_q || !d_scale || rows <= 0 || hidden <= 0) return TIA_EINVAL;
    if (!is_half(dtype)) return TIA_EINVAL;
    if ((hidden & 15) != 0 || hidden > 8192) return TIA_ESIZE;
    if (misaligned({d_x, d_q, d_scale})) return TIA_EINVAL;
    const long blocks = (rows + ET / 64 - 1) / (ET / 64);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    for_row_width(dtype, hidden, [&](auto bf, auto vpl) {
        hipLaunchKernelGGL((act_rows_kernel<F, decltype(bf)::value, SWIGLU, decltype(vpl)::value>), dim3((unsigned)blocks), dim3(ET), 0, (hipStream_t)stream,
                           static_cast<const unsigned short*>(d_x), (long)rows, (int)hidden, static_cast<typename F::code_t*>(d_q),
                           d_scale);
    });
    return launched();
}

template <class F, bool SWIGLU>
int act_rows_smooth(const void* d_x, const float* d_inv_smooth, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype,
                    void* stream) {
    if (!d_x || !d_inv_smooth || !d_q || !d_scale || rows <= 0 || hidden <= 0) return TIA_EINVAL;
    if (!is_half(dtype)) return TIA_EINVAL;
    if ((hidden & 15) != 0 || hidden > 8192) return TIA_ESIZE;
    if (misaligned({d_x, d_inv_smooth, d_q, d_scale})) return TIA_EINVAL;
    const long blocks = (rows + ET / 64 - 1) / (ET / 64);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    for_row_width(dtype, hidden, [&](auto bf, auto vpl) {
        hipLaunchKernelGGL((act_rows_smooth_kernel<F, decltype(bf)::value, SWIGLU, decltype(vpl)::value>), dim3((unsigned)blocks), dim3(ET), 0,
                           (hipStream_t)stream, static_cast<const unsigned short*>(d_x), d_inv_smooth, (long)rows, (int)hidden,
                           static_cast<typename F::code_t*>(d_q), d_scale);
    });
    return launched();
}

}  // namespace

}  // namespace tia::q8
