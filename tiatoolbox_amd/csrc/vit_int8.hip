// The Vision Transformer linear layers on the INT8 matrix instruction (models/architecture/vit_fused.py, linear_dtype="int8";
// DESIGN 4.38).  W8A8, symmetric, one scale per token and one per output channel:
//   one row     v[0 .. K) float32:  amax = max |v| (a NaN in the row makes amax NaN);  inv = 127 / amax and s = amax / 127, one
//               float32 division each (amax == 0: inv = s = 1);  q[k] = clamp(rne(v[k] * inv), -127, 127), the product in float32, a
//               NaN product -> code 0; the code -128 is never made.  Stored as q (K bytes of int8) and s (one float32)
//   non-finite  a row holding NaN has s = NaN, a row holding +-inf (and no NaN) s = +inf: every output of that token is non-finite
//   weights     one row per output channel, quantised once from the float32 (LayerScale-folded, SwiGLU-padded) weights
//   activations one row per token, quantised from the float32 value the producing kernel holds, before any rounding to half
//   GEMM        acc[r,o] = sum_k qa[r,k] qw[o,k] exactly in int32 (K <= 65536: K 127^2 < 2^31);
//               y[r,o] = half_rne(float(acc) * sa[r] * sw[o] + bias[o] (+ float32(residual[r,o]))), float(acc) to nearest even
// on v_mfma_i32_16x16x64_i8, two instructions per 128-deep K-step.
//   linear_int8_rows          the GEMM
//   linear_int8_pack_weights  float32 [N, K] -> codes [N, K] + scales [N]
//   layernorm_rows_qi8        LayerNorm of half rows -> codes + scales            (feeds qkv and fc1)
//   gelu_rows_qi8             half fc1 output -> exact GELU in float32 -> codes + scales      (feeds fc2)
//   swiglu_rows_qi8           half packed fc1 output [rows, 2H] -> silu(gate) * value -> codes [rows, H] + scales
// The arithmetic of the three producers up to the float32 value is that of the _h kernels of vit_rows.hip.  The kernels and their
// launchers are vit_quant_rows.hpp's (shared with vit_fp8.hip), instantiated here for the format Int8.
#include "vit_quant_rows.hpp"

namespace tia::q8 {

using v4i = __attribute__((ext_vector_type(4))) int;

struct Int8 {
    using code_t = signed char;
    using acc_t = v4i;
    static constexpr int64_t K_MAX = 65536;  // K 127^2 stays inside int32
    static constexpr float MAX = 127.0f;

    static __device__ __forceinline__ acc_t zero() { return acc_t{0, 0, 0, 0}; }
    // the instruction takes 16 bytes per lane and operand: the low piece, then the high one (the int32 sum is exact, whatever the order)
    template <int P>
    static __device__ __forceinline__ v4i piece(const v8i& f) {
        return __builtin_shufflevector(f, f, 4 * P, 4 * P + 1, 4 * P + 2, 4 * P + 3);
    }
    static __device__ __forceinline__ acc_t step(const v8i& w, const v8i& t, acc_t acc) {
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(piece<0>(w), piece<0>(t), acc, 0, 0, 0);
        return __builtin_amdgcn_mfma_i32_16x16x64_i8(piece<1>(w), piece<1>(t), acc, 0, 0, 0);
    }
    // the larger of two magnitudes; a NaN on either side stays (fmaxf would drop it)
    static __device__ __forceinline__ float amax(float a, float b) { return (b > a || b != b) ? b : a; }
    // two correctly rounded float32 divisions; an all-zero row keeps scale 1.  A NaN amax gives inv = s = NaN, an infinite one
    // inv = 0 and s = inf.
    static __device__ __forceinline__ void row_scales(float amax, float& inv, float& s) {
        inv = amax == 0.0f ? 1.0f : MAX / amax;
        s = amax == 0.0f ? 1.0f : amax / MAX;
    }
    // round to nearest even, a NaN -> 0, clamped to +-127
    static __device__ __forceinline__ unsigned code(float x) {
        float q = rintf(x);
        q = q != q ? 0.0f : q;
        q = fminf(fmaxf(q, -MAX), MAX);
        return (unsigned)(int)q & 0xffu;
    }
};

namespace {

// ---- calibration statistics -----------------------------------------------------------------------------------------------------
// amax[j] = max(amax[j], max over rows |v[r, j]|) of the float32 values v a producer above holds.  Magnitudes travel as the bit
// pattern of |v|, compared as unsigned integers: the order of the non-negative floats, with every NaN above +inf, so a NaN in a column
// stays there.  A workgroup keeps the column maxima of all the rows it visits in LDS (vector v of a row at [j][v], so that a wave's
// 64 lanes touch 64 consecutive words) and ends with one atomic maximum per column that saw anything but zeros.
constexpr int ABSMAX_BLOCKS = 1024;  // at most this many workgroups; a wave strides over the rows

__device__ __forceinline__ void column_max_clear(unsigned* cm, int c) {
    for (int i = threadIdx.x; i < c; i += ET) cm[i] = 0u;
    __syncthreads();
}

template <int VPL>
__device__ __forceinline__ void column_max_row(const float (&f)[VPL][8], int lane, int cv, unsigned* cm) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
#pragma unroll
            for (int j = 0; j < 8; ++j) atomicMax(cm + j * cv + v, __float_as_uint(f[i][j]) & 0x7fffffffu);
        }
    }
}

__device__ __forceinline__ void column_max_flush(const unsigned* cm, int c, unsigned* __restrict__ amax) {
    __syncthreads();
    const int cv = c >> 3;
    for (int col = threadIdx.x; col < c; col += ET) {
        const unsigned m = cm[(col & 7) * cv + (col >> 3)];
        if (m != 0u) atomicMax(amax + col, m);
    }
}

template <bool BF, int VPL>
__global__ __launch_bounds__(ET) void layernorm_rows_absmax_kernel(const unsigned short* __restrict__ x, long stride,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    float eps, long rows, int c, unsigned* __restrict__ amax) {
    __shared__ unsigned cm[VPL * 512];
    column_max_clear(cm, c);
    const int lane = threadIdx.x & 63;
    for (long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * (ET / 64)) {
        float f[VPL][8];
        layernorm_row_values<BF, VPL>(x + row * stride, gamma, beta, eps, c, lane, f);
        column_max_row<VPL>(f, lane, c >> 3, cm);
    }
    column_max_flush(cm, c, amax);
}

template <bool BF, bool SWIGLU, int VPL>
__global__ __launch_bounds__(ET) void act_rows_absmax_kernel(const unsigned short* __restrict__ x, long rows, int hidden,
                                                              unsigned* __restrict__ amax) {
    __shared__ unsigned cm[VPL * 512];
    column_max_clear(cm, hidden);
    const int lane = threadIdx.x & 63;
    for (long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * (ET / 64)) {
        float f[VPL][8];
        act_row_values<BF, SWIGLU, VPL>(x + row * (SWIGLU ? 2L : 1L) * hidden, hidden, lane, f);
        column_max_row<VPL>(f, lane, hidden >> 3, cm);
    }
    column_max_flush(cm, hidden, amax);
}

inline unsigned absmax_blocks(int64_t rows) {
    const int64_t blocks = (rows + ET / 64 - 1) / (ET / 64);
    return (unsigned)(blocks < ABSMAX_BLOCKS ? blocks : ABSMAX_BLOCKS);
}

inline int layernorm_rows_absmax(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, float* d_amax,
                                 int64_t rows, int64_t c, int32_t dtype, void* stream) {
    if (!d_x || !d_gamma || !d_beta || !d_amax || rows <= 0 || c <= 0 || !(eps >= 0.0f)) return TIA_EINVAL;
    if (!is_half(dtype)) return TIA_EINVAL;
    if ((c & 15) != 0 || c > 8192) return TIA_ESIZE;
    if (row_stride < c || (row_stride & 7) != 0) return TIA_EINVAL;
    if (misaligned({d_x, d_gamma, d_beta, d_amax})) return TIA_EINVAL;
    if (rows > (int64_t(1) << 40)) return TIA_ESIZE;
    for_row_width(dtype, c, [&](auto bf, auto vpl) {
        hipLaunchKernelGGL((layernorm_rows_absmax_kernel<decltype(bf)::value, decltype(vpl)::value>), dim3(absmax_blocks(rows)), dim3(ET), 0,
                           (hipStream_t)stream, static_cast<const unsigned short*>(d_x), (long)row_stride, d_gamma, d_beta, eps, (long)rows,
                           (int)c, reinterpret_cast<unsigned*>(d_amax));
    });
    return launched();
}

template <bool SWIGLU>
int act_rows_absmax(const void* d_x, float* d_amax, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    if (!d_x || !d_amax || rows <= 0 || hidden <= 0) return TIA_EINVAL;
    if (!is_half(dtype)) return TIA_EINVAL;
    if ((hidden & 15) != 0 || hidden > 8192) return TIA_ESIZE;
    if (misaligned({d_x, d_amax})) return TIA_EINVAL;
    if (rows > (int64_t(1) << 40)) return TIA_ESIZE;
    for_row_width(dtype, hidden, [&](auto bf, auto vpl) {
        hipLaunchKernelGGL((act_rows_absmax_kernel<decltype(bf)::value, SWIGLU, decltype(vpl)::value>), dim3(absmax_blocks(rows)), dim3(ET), 0,
                           (hipStream_t)stream, static_cast<const unsigned short*>(d_x), (long)rows, (int)hidden,
                           reinterpret_cast<unsigned*>(d_amax));
    });
    return launched();
}

}  // namespace

}  // namespace tia::q8

using tia::q8::Int8;

extern "C" int tia_linear_int8_serves(int64_t rows, int64_t n, int64_t k) { return tia::q8::serves<Int8>(rows, n, k); }

extern "C" int tia_linear_int8_rows(const void* d_a, const float* d_sa, const void* d_w, const float* d_sw, const float* d_bias,
                                    const void* d_residual, void* d_y, int64_t rows, int64_t n, int64_t k, int32_t dtype, void* stream) {
    return tia::q8::linear_rows<Int8>(d_a, d_sa, d_w, d_sw, d_bias, d_residual, d_y, rows, n, k, dtype, stream);
}

extern "C" int tia_linear_int8_pack_weights(const float* d_w, int64_t n, int64_t k, void* d_q, float* d_scale, void* stream) {
    return tia::q8::pack_weights<Int8>(d_w, n, k, d_q, d_scale, stream);
}

extern "C" int tia_layernorm_rows_qi8(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, void* d_q,
                                      float* d_scale, int64_t rows, int64_t c, int32_t dtype, void* stream) {
    return tia::q8::layernorm_rows<Int8>(d_x, row_stride, d_gamma, d_beta, eps, d_q, d_scale, rows, c, dtype, stream);
}

extern "C" int tia_gelu_rows_qi8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    return tia::q8::act_rows<Int8, false>(d_x, d_q, d_scale, rows, hidden, dtype, stream);
}

extern "C" int tia_swiglu_rows_qi8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    return tia::q8::act_rows<Int8, true>(d_x, d_q, d_scale, rows, hidden, dtype, stream);
}

// ---- per-input-channel smoothing of fc2's input, and the calibration statistics of all three producer sites --------

extern "C" int tia_gelu_rows_qi8_smooth(const void* d_x, const float* d_inv_smooth, void* d_q, float* d_scale, int64_t rows,
                                         int64_t hidden, int32_t dtype, void* stream) {
    return tia::q8::act_rows_smooth<Int8, false>(d_x, d_inv_smooth, d_q, d_scale, rows, hidden, dtype, stream);
}

extern "C" int tia_swiglu_rows_qi8_smooth(const void* d_x, const float* d_inv_smooth, void* d_q, float* d_scale, int64_t rows,
                                           int64_t hidden, int32_t dtype, void* stream) {
    return tia::q8::act_rows_smooth<Int8, true>(d_x, d_inv_smooth, d_q, d_scale, rows, hidden, dtype, stream);
}

extern "C" int tia_layernorm_rows_absmax_h(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps,
                                           float* d_amax, int64_t rows, int64_t c, int32_t dtype, void* stream) {
    return tia::q8::layernorm_rows_absmax(d_x, row_stride, d_gamma, d_beta, eps, d_amax, rows, c, dtype, stream);
}

extern "C" int tia_gelu_rows_absmax_h(const void* d_x, float* d_amax, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    return tia::q8::act_rows_absmax<false>(d_x, d_amax, rows, hidden, dtype, stream);
}

extern "C" int tia_swiglu_rows_absmax_h(const void* d_x, float* d_amax, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    return tia::q8::act_rows_absmax<true>(d_x, d_amax, rows, hidden, dtype, stream);
}
