// What the row kernels over half (fp16 / bf16) activations share: a 16-byte vector of 8 halves to and from float32, 8 float32 from
// two 16-byte loads, the folds over a wave by lane exchanges (no LDS, no barrier) and silu.  vit_rows.hip, vit_classifier.hip,
// vit_f32.hip, cnn_epilogue_h.hip and the quantising kernels of vit_quant_rows.hpp take them from here.  The spelling
// of each is the one that leaves every kernel's instruction stream as it was (pack8: the loop form of cnn_epilogue_h.hip).
#pragma once
#include "conv_device.hpp"
#include "wide_io.hpp"

namespace tia {

template <bool BF>
__device__ __forceinline__ void unpack8(const v4u& v, float (&f)[8]) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = half_to_f32<BF>((unsigned short)(w[i] & 0xffffu));
        f[2 * i + 1] = half_to_f32<BF>((unsigned short)(w[i] >> 16));
    }
}
template <bool BF>
__device__ __forceinline__ v4u pack8(const float (&f)[8]) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (unsigned)f32_to_half<BF>(f[2 * i]) | ((unsigned)f32_to_half<BF>(f[2 * i + 1]) << 16);
    v4u v;
    v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
    return v;
}
__device__ __forceinline__ void load8_f32(const float* p, float (&f)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// silu(t) = t / (1 + exp(-t)), written so that no exponential overflows: with e = exp(-|t|) in (0, 1] it is t / (1 + e) for t >= 0
// and t e / (1 + e) for t < 0 -- a gate of -100 gives the tiny value it should (or a signed zero), never inf / inf.  expf and the
// division are the correctly rounded ones (no fast-math): a few float32 units in all.
__device__ __forceinline__ float silu_f32(float t) {
    const float e = expf(-fabsf(t));
    const float num = t >= 0.0f ? t : t * e;
    return num / (1.0f + e);
}

}  // namespace tia
