// The Vision Transformer linear layers on the FP8 matrix instruction (models/architecture/vit_fused.py, linear_dtype="float8_e4m3";
// DESIGN 4.34).  Row x column scaled FP8, not MXFP8:
//   format      OCP e4m3fn (largest finite value 448, no infinities; NOT the MI300 fnuz encoding); float32 -> code is round to nearest
//               even, saturating at +-448 (fp8_e4m3.hpp)
//   one row     v[0 .. K) float32:  amax = max |v|;  inv = 448 / amax and s = amax / 448, one float32 division each (amax == 0:
//               inv = s = 1);  q[k] = e4m3(v[k] * inv), the product in float32;  stored as q (K bytes) and s (one float32)
//   weights     one row per output channel, quantised once from the float32 (LayerScale-folded, SwiGLU-padded) weights
//   activations one row per token, quantised from the float32 value the producing kernel holds, before any rounding to half
//   GEMM        acc[r,o] = sum_k qa[r,k] qw[o,k] (exact products, float32 accumulation in any order);
//               y[r,o] = half_rne(acc * sa[r] * sw[o] + bias[o] (+ float32(residual[r,o])))
// on v_mfma_scale_f32_16x16x128_f8f6f4 with both block-scale operands the constant 1.0 (E8M0 127).
//   linear_fp8_rows          the GEMM
//   linear_fp8_pack_weights  float32 [N, K] -> codes [N, K] + scales [N]
//   layernorm_rows_q8        LayerNorm of half rows -> codes + scales            (feeds qkv and fc1)
//   gelu_rows_q8             half fc1 output -> exact GELU in float32 -> codes + scales      (feeds fc2)
//   swiglu_rows_q8           half packed fc1 output [rows, 2H] -> silu(gate) * value -> codes [rows, H] + scales
// The arithmetic of the three producers up to the float32 value is that of the _h kernels of vit_rows.hip.  The kernels and their
// launchers are vit_quant_rows.hpp's (shared with vit_int8.hip), instantiated here for the format E4m3.
#include "fp8_e4m3.hpp"
#include "vit_quant_rows.hpp"

namespace tia::q8 {

using v4f = __attribute__((ext_vector_type(4))) float;

struct E4m3 {
    using code_t = unsigned char;
    using acc_t = v4f;
    static constexpr int64_t K_MAX = 1 << 20;
    static constexpr float MAX = 448.0f;
    static constexpr int E8M0_ONE = 0x7f7f7f7f;  // block scale 2^0 in every byte the scale selector can pick

    static __device__ __forceinline__ acc_t zero() { return acc_t{0.0f, 0.0f, 0.0f, 0.0f}; }
    // one instruction on the lane's 32 bytes
    static __device__ __forceinline__ acc_t step(const v8i& w, const v8i& t, const acc_t& acc) {
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, t, acc, 0, 0, 0, E8M0_ONE, 0, E8M0_ONE);
    }
    static __device__ __forceinline__ float amax(float a, float b) { return fmaxf(a, b); }
    // two correctly rounded float32 divisions; an all-zero row keeps scale 1
    static __device__ __forceinline__ void row_scales(float amax, float& inv, float& s) {
        inv = amax > 0.0f ? MAX / amax : 1.0f;
        s = amax > 0.0f ? amax / MAX : 1.0f;
    }
    static __device__ __forceinline__ unsigned code(float x) { return f32_to_e4m3(x); }
};

}  // namespace tia::q8

using tia::q8::E4m3;

extern "C" int tia_linear_fp8_serves(int64_t rows, int64_t n, int64_t k) { return tia::q8::serves<E4m3>(rows, n, k); }

extern "C" int tia_linear_fp8_rows(const void* d_a, const float* d_sa, const void* d_w, const float* d_sw, const float* d_bias,
                                   const void* d_residual, void* d_y, int64_t rows, int64_t n, int64_t k, int32_t dtype, void* stream) {
    return tia::q8::linear_rows<E4m3>(d_a, d_sa, d_w, d_sw, d_bias, d_residual, d_y, rows, n, k, dtype, stream);
}

extern "C" int tia_linear_fp8_pack_weights(const float* d_w, int64_t n, int64_t k, void* d_q, float* d_scale, void* stream) {
    return tia::q8::pack_weights<E4m3>(d_w, n, k, d_q, d_scale, stream);
}

extern "C" int tia_layernorm_rows_q8(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, void* d_q,
                                     float* d_scale, int64_t rows, int64_t c, int32_t dtype, void* stream) {
    return tia::q8::layernorm_rows<E4m3>(d_x, row_stride, d_gamma, d_beta, eps, d_q, d_scale, rows, c, dtype, stream);
}

extern "C" int tia_gelu_rows_q8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    return tia::q8::act_rows<E4m3, false>(d_x, d_q, d_scale, rows, hidden, dtype, stream);
}

extern "C" int tia_swiglu_rows_q8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    return tia::q8::act_rows<E4m3, true>(d_x, d_q, d_scale, rows, hidden, dtype, stream);
}
