// The two streaming passes between the convolutions of a plain-encoder / concat-skip UNet (gfx950, NHWC, HBM-bound), written once
// for float32 (cnn_epilogue.hip) and fp16 / bf16 (cnn_epilogue_h.hip):
//   avgpool2x2        : y[b, oy, ox, :] = (((x00 + x01) + x10) + x11) * 0.25        AvgPool2d(2, stride=2); a last odd row / column is not read
//   upsample2x_concat : out[b, Y, X, :] = act(cat(x[b, Y/2, X/2, :], y[b, Y, X, :]))  nearest x2 up-sampling + channel concatenation
// `V` is the 16-byte vector of the element type (N elements; unpack to / pack from float32 lanes: Vec<T> there, HalfVec<BF> here).
// One thread per vector, 16 bytes per access, consecutive lanes walk the channels and then the pixels, so every access of a wave
// covers whole pixels' worth of contiguous bytes.  blockIdx.x is a row of the SMALLER map (64-bit offsets from there on: a tensor may
// exceed 2^31 elements), blockIdx.y * 256 + threadIdx.x the vector within that row.  No LDS, no atomics.
#pragma once
#include "wide_io.hpp"

#pragma clang fp contract(off)

namespace tia {

constexpr int GT = 256;  // threads per workgroup

// x00 x01 / x10 x11 = the window's rows 2 oy, 2 oy + 1 and columns 2 ox, 2 ox + 1.  The sums are rounded one by one in float32 in
// exactly this order (the order of torch's avg_pool2d; the pairwise (x00 + x01) + (x10 + x11) is another function), then one
// multiplication by 0.25 (exact but for underflow) and, for halves, ONE rounding.  Four elements read per element written.
template <class V>
__global__ __launch_bounds__(GT) void avgpool2x2_kernel(const v4u* __restrict__ x, int h, int w, int cv, int ho, int wo,
                                                         v4u* __restrict__ y) {
    constexpr int N = V::N;
    const int j = blockIdx.y * GT + threadIdx.x;
    if (j >= wo * cv) return;
    const long row = blockIdx.x;  // b * ho + oy
    const long b = row / ho;
    const int oy = (int)(row - b * ho);
    const int ox = j / cv, c = j - ox * cv;
    const long rs = (long)w * cv;  // vectors per input row
    const v4u* p = x + ((b * h + 2 * oy) * w + 2 * ox) * (long)cv + c;
    const v4u r00 = p[0], r01 = p[cv], r10 = p[rs], r11 = p[rs + cv];
    float s[8], t[8];
    V::unpack(r00, s);
    V::unpack(r01, t);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = s[k] + t[k];
    V::unpack(r10, t);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = s[k] + t[k];
    V::unpack(r11, t);
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = (s[k] + t[k]) * 0.25f;
    y[row * ((long)wo * cv) + j] = V::pack(s);
}

// One thread per vector of an INPUT pixel's concatenated channels: a vector of x is read once and written to the 2 x 2 output block
// above it, a vector of y's 2 x 2 block is read four times and written four times.  ACT: relu(v * scale[ch] + shift[ch]) on the way
// (product and sum rounded separately in float32; halves: widened first, ONE rounding at the end); without it the 16 bytes are
// copied as they are.  The x / y branch splits a wave at channel-group boundaries only; the four stores are common to both.
template <class V, bool ACT>
__global__ __launch_bounds__(GT) void upsample2x_concat_kernel(const v4u* __restrict__ x, const v4u* __restrict__ y, int w, int cxv,
                                                                int cyv, const float4* __restrict__ scale,
                                                                const float4* __restrict__ shift, v4u* __restrict__ out) {
    constexpr int N = V::N;
    const int cov = cxv + cyv;
    const int j = blockIdx.y * GT + threadIdx.x;
    if (j >= w * cov) return;
    const long row = blockIdx.x;  // b * h + yy: the output rows are 2 * row and 2 * row + 1
    const int xx = j / cov, v = j - xx * cov;
    const long orow = 2L * w;  // pixels per output row
    v4u r[4];
    if (v < cxv) {
        r[0] = r[1] = r[2] = r[3] = x[(row * w + xx) * cxv + v];
    } else {
        const v4u* yp = y + (2 * row * orow + 2 * xx) * cyv + (v - cxv);
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = yp[((q >> 1) * orow + (q & 1)) * cyv];
    }
    if (ACT) {
        float sc[8], sh[8];
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const float4 s = scale[v * (N / 4) + i], t = shift[v * (N / 4) + i];
            sc[4 * i] = s.x, sc[4 * i + 1] = s.y, sc[4 * i + 2] = s.z, sc[4 * i + 3] = s.w;
            sh[4 * i] = t.x, sh[4 * i + 1] = t.y, sh[4 * i + 2] = t.z, sh[4 * i + 3] = t.w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float f[8];
            V::unpack(r[q], f);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                float a = f[k] * sc[k];
                a = a + sh[k];
                f[k] = a > 0.0f ? a : 0.0f;
            }
            r[q] = V::pack(f);
        }
    }
    v4u* op = out + (2 * row * orow + 2 * xx) * cov + v;
#pragma unroll
    for (int q = 0; q < 4; ++q) op[((q >> 1) * orow + (q & 1)) * cov] = r[q];
}

static inline bool glue_misaligned(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr,
                                   const void* e = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(e)) & 15) != 0;
}

// The entry points' bodies: every check comes before the launch, so nothing is launched on an error return.
template <class V>
int launch_avgpool2x2(const void* d_x, void* d_y, int64_t n, int64_t h, int64_t w, int64_t c, hipStream_t st) {
    if (!d_x || !d_y || n <= 0 || h < 2 || w < 2 || c <= 0) return TIA_EINVAL;
    if (c % V::N != 0) return TIA_ESIZE;  // 16 bytes per access
    if (glue_misaligned(d_x, d_y)) return TIA_EINVAL;
    const long cv = c / V::N, ho = h / 2, wo = w / 2;
    const long per_row = (wo * cv + GT - 1) / GT;
    if (n * ho > 0x7fffffffL || per_row > 65535 || h > 0x7fffffffL || w > 0x7fffffffL) return TIA_ESIZE;
    hipLaunchKernelGGL(avgpool2x2_kernel<V>, dim3((unsigned)(n * ho), (unsigned)per_row), dim3(GT), 0, st, (const v4u*)d_x, (int)h, (int)w,
                       (int)cv, (int)ho, (int)wo, (v4u*)d_y);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

template <class V>
int launch_upsample2x_concat(const void* d_x, const void* d_y, const float* d_scale, const float* d_shift, void* d_out, int64_t n,
                             int64_t h, int64_t w, int64_t cx, int64_t cy, hipStream_t st) {
    if (!d_x || !d_y || !d_out || n <= 0 || h <= 0 || w <= 0 || cx <= 0 || cy <= 0) return TIA_EINVAL;
    if ((d_scale == nullptr) != (d_shift == nullptr)) return TIA_EINVAL;
    if (cx % V::N != 0 || cy % V::N != 0) return TIA_ESIZE;  // 16 bytes per access, the seam between x's and y's channels included
    if (glue_misaligned(d_x, d_y, d_out, d_scale, d_shift)) return TIA_EINVAL;
    const long cxv = cx / V::N, cyv = cy / V::N;
    const long per_row = (w * (cxv + cyv) + GT - 1) / GT;
    if (n * h > 0x7fffffffL || per_row > 65535 || w > 0x3fffffffL) return TIA_ESIZE;
    const auto kernel = d_scale ? upsample2x_concat_kernel<V, true> : upsample2x_concat_kernel<V, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(n * h), (unsigned)per_row), dim3(GT), 0, st, (const v4u*)d_x, (const v4u*)d_y, (int)w,
                       (int)cxv, (int)cyv, (const float4*)d_scale, (const float4*)d_shift, (v4u*)d_out);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

}  // namespace tia
