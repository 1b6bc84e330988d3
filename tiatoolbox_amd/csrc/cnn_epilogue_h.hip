// The glue between the half-precision convolutions of the UNet (fp16 / bf16 NHWC activations), HBM-bound:
//   upsample2x_add_act : out[b, Y, X, :] = act(x[b, Y/2, X/2, :] + y[b, Y, X, :])    half in, half out
//   head 1x1           : y[p][o] = bias[o] + sum_c w[o][c] * pre(x[p][c])            half in, float32 logits out
// The half forms of tia_upsample2x_add_act_nhwc_f32 / tia_conv1x1_head_nhwc_f32 (cnn_epilogue.hip).  16 bytes per lane and
// access (8 halves), float32 arithmetic with every step rounded on its own (contraction off: the order of the unfused torch
// ops), ONE round-to-nearest-even to half at the end, 64-bit element offsets (a tensor may exceed 2^31 bytes).
#include "conv_device.hpp"
#include "wide_io.hpp"

#pragma clang fp contract(off)

namespace {

using namespace tia;

constexpr int ET = 256;

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

// One thread per 8 channels of an INPUT pixel: it reads that vector once and produces the 2 x 2 output block above it (four
// reads of the skip view, four stores).  blockIdx.x = input row b * h + yy (so the two output rows are 2 * row and 2 * row + 1),
// blockIdx.y * ET + threadIdx.x = xx * cv + vector within the pixel: consecutive lanes walk the channels, then the pixels --
// every access of a wave covers whole pixels' worth of contiguous bytes (the two stores of an output row interleave pixel-wise).
// Bytes per output element: 2 (y) + 2 (out) + 0.5 (x) = 4.5.
template <bool BF, bool ACT>
__global__ __launch_bounds__(ET) void upsample2x_add_h_kernel(const v4u* __restrict__ x, const unsigned short* __restrict__ y, long y_sb,
                                                               long y_sy, int h, int w, int cv, const float4* __restrict__ scale,
                                                               const float4* __restrict__ shift, v4u* __restrict__ out) {
    const int j = blockIdx.y * ET + threadIdx.x;
    if (j >= w * cv) return;
    const long row = blockIdx.x;
    const int b = (int)(row / h), yy = (int)(row - (long)b * h);
    const int xx = j / cv, c = j - xx * cv;
    float a[8];
    unpack8<BF>(x[row * ((long)w * cv) + j], a);
    float sc[8], sh[8];
    if (ACT) {
        const float4 s0 = scale[2 * c], s1 = scale[2 * c + 1], t0 = shift[2 * c], t1 = shift[2 * c + 1];
        sc[0] = s0.x, sc[1] = s0.y, sc[2] = s0.z, sc[3] = s0.w, sc[4] = s1.x, sc[5] = s1.y, sc[6] = s1.z, sc[7] = s1.w;
        sh[0] = t0.x, sh[1] = t0.y, sh[2] = t0.z, sh[3] = t0.w, sh[4] = t1.x, sh[5] = t1.y, sh[6] = t1.z, sh[7] = t1.w;
    }
    const unsigned short* yp = y + (long)b * y_sb + (long)(2 * yy) * y_sy + ((long)(2 * xx) * cv + c) * 8;
    v4u* op = out + (2 * row * (2L * w) + 2 * xx) * cv + c;
    v4u r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = *reinterpret_cast<const v4u*>(yp + (q >> 1) * y_sy + (long)(q & 1) * cv * 8);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float f[8];
        unpack8<BF>(r[q], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float v = a[k] + f[k];
            if (ACT) {
                v = v * sc[k];
                v = v + sh[k];
                v = v > 0.0f ? v : 0.0f;
            }
            f[k] = v;
        }
        op[(q >> 1) * (2L * w) * cv + (q & 1) * cv] = pack8<BF>(f);
    }
}

// Class head on half activations: 8 lanes share a pixel (8 of its 64 channels each: a wave reads 8 pixels = 1 KB contiguous),
// multiply by their slice of the float32 weights and fold the 8 partial sums with a butterfly of lane exchanges; lanes
// 0 .. COUT-1 of each 8 write the pixel's float32 logits (8 * COUT contiguous floats per wave).  128 B read + 4 * COUT written
// per pixel.
template <bool BF, int COUT>
__global__ __launch_bounds__(ET) void head1x1_h_kernel(const v4u* __restrict__ x, long npix, const float* __restrict__ w,
                                                        const float* __restrict__ bias, const float* __restrict__ ps,
                                                        const float* __restrict__ pt, float* __restrict__ y) {
    const int lane = threadIdx.x & 63, q = lane & 7, sub = lane >> 3;
    float wr[COUT][8];
#pragma unroll
    for (int o = 0; o < COUT; ++o)
#pragma unroll
        for (int i = 0; i < 8; ++i) wr[o][i] = w[o * 64 + 8 * q + i];
    float sc[8], sh[8];
    const bool pre = ps != nullptr;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = pre ? ps[8 * q + i] : 1.0f;
        sh[i] = pre ? pt[8 * q + i] : 0.0f;
    }
    float bo = 0.0f;
    if (bias && q < COUT) bo = bias[q];
    const long groups = (npix + 7) / 8;
    const long wave = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6), waves = (long)gridDim.x * (ET / 64);
    constexpr int U = 4;  // groups in flight per wave
    for (long g0 = wave * U; g0 < groups; g0 += waves * U) {
        v4u v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long pix = (g0 + u) * 8 + sub;
            v4u z;
            z.x = z.y = z.z = z.w = 0u;
            v[u] = pix < npix ? x[pix * 8 + q] : z;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float a[8];
            unpack8<BF>(v[u], a);
            if (pre) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {  // rounded like batch_norm, then relu
                    float t = a[i] * sc[i];
                    t = t + sh[i];
                    a[i] = t > 0.0f ? t : 0.0f;
                }
            }
            float part[COUT];
#pragma unroll
            for (int o = 0; o < COUT; ++o) {
                float t = a[0] * wr[o][0];
#pragma unroll
                for (int i = 1; i < 8; ++i) t = fmaf(a[i], wr[o][i], t);
                part[o] = t;
            }
#pragma unroll
            for (int m = 1; m < 8; m <<= 1)
#pragma unroll
                for (int o = 0; o < COUT; ++o) part[o] += __shfl_xor(part[o], m, 64);
            float mine = part[0];
#pragma unroll
            for (int o = 1; o < COUT; ++o) mine = q == o ? part[o] : mine;
            const long pix = (g0 + u) * 8 + sub;
            if (q < COUT && pix < npix) y[pix * COUT + q] = mine + bo;
        }
    }
}

template <bool BF, int COUT>
void launch_head_h(const void* x, long npix, const float* w, const float* bias, const float* ps, const float* pt, float* y, hipStream_t st) {
    long blocks = ((npix + 7) / 8 + 15) / 16;  // 4 waves x 4 groups per pass
    if (blocks > 256L * 16) blocks = 256L * 16;
    hipLaunchKernelGGL((head1x1_h_kernel<BF, COUT>), dim3((unsigned)blocks), dim3(ET), 0, st, (const v4u*)x, npix, w, bias, ps, pt, y);
}

template <bool BF>
void launch_head_h_cout(int cout, const void* x, long npix, const float* w, const float* bias, const float* ps, const float* pt, float* y,
                        hipStream_t st) {
    switch (cout) {
        case 1: launch_head_h<BF, 1>(x, npix, w, bias, ps, pt, y, st); break;
        case 2: launch_head_h<BF, 2>(x, npix, w, bias, ps, pt, y, st); break;
        case 3: launch_head_h<BF, 3>(x, npix, w, bias, ps, pt, y, st); break;
        case 4: launch_head_h<BF, 4>(x, npix, w, bias, ps, pt, y, st); break;
        case 5: launch_head_h<BF, 5>(x, npix, w, bias, ps, pt, y, st); break;
        case 6: launch_head_h<BF, 6>(x, npix, w, bias, ps, pt, y, st); break;
        case 7: launch_head_h<BF, 7>(x, npix, w, bias, ps, pt, y, st); break;
        default: launch_head_h<BF, 8>(x, npix, w, bias, ps, pt, y, st); break;
    }
}

}  // namespace

extern "C" int tia_upsample2x_add_act_nhwc_h(const void* d_x, const void* d_y, int64_t y_image_stride, int64_t y_row_stride,
                                             const float* d_scale, const float* d_shift, void* d_out, int64_t n, int64_t h, int64_t w,
                                             int64_t c, int32_t dtype, void* stream) {
    if (!d_x || !d_y || !d_out || n <= 0 || h <= 0 || w <= 0 || c <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((d_scale == nullptr) != (d_shift == nullptr)) return TIA_EINVAL;
    if ((c & 7) != 0) return TIA_ESIZE;  // 8 halves per access
    if ((reinterpret_cast<uintptr_t>(d_scale) | reinterpret_cast<uintptr_t>(d_shift)) & 15) return TIA_EINVAL;
    if ((y_image_stride & 7) != 0 || (y_row_stride & 7) != 0 || y_row_stride < 2 * w * c) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y) | reinterpret_cast<uintptr_t>(d_out)) & 15) return TIA_EINVAL;
    const long cv = c / 8;
    const long per_row = (w * cv + ET - 1) / ET;
    if (n * h > 0x7fffffffL || per_row > 65535 || w * cv > 0x7fffffffL || 2 * h > 0x7fffffffL) return TIA_ESIZE;
    const dim3 grid((unsigned)(n * h), (unsigned)per_row);
    hipStream_t st = (hipStream_t)stream;
    const bool bf = dtype == TIA_DT_BF16, act = d_scale != nullptr;
    using Kernel = void (*)(const v4u*, const unsigned short*, long, long, int, int, int, const float4*, const float4*, v4u*);
    const Kernel kernels[2][2] = {{upsample2x_add_h_kernel<false, false>, upsample2x_add_h_kernel<false, true>},
                                  {upsample2x_add_h_kernel<true, false>, upsample2x_add_h_kernel<true, true>}};
    hipLaunchKernelGGL(kernels[bf][act], grid, dim3(ET), 0, st, (const v4u*)d_x, (const unsigned short*)d_y, (long)y_image_stride,
                       (long)y_row_stride, (int)h, (int)w, (int)cv, (const float4*)d_scale, (const float4*)d_shift, (v4u*)d_out);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_conv1x1_head_nhwc_h(const void* d_x, int64_t npix, const float* d_w, const float* d_bias, const float* d_pre_scale,
                                       const float* d_pre_shift, int32_t cout, int32_t dtype, float* d_y, void* stream) {
    if (!d_x || !d_w || !d_y || npix <= 0 || cout < 1 || cout > 8 || ((d_pre_scale == nullptr) != (d_pre_shift == nullptr))) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_x) & 15) return TIA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == TIA_DT_BF16) launch_head_h_cout<true>(cout, d_x, npix, d_w, d_bias, d_pre_scale, d_pre_shift, d_y, st);
    else launch_head_h_cout<false>(cout, d_x, npix, d_w, d_bias, d_pre_scale, d_pre_shift, d_y, st);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
