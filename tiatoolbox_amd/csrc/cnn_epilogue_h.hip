// The glue between the half-precision convolutions of the UNet and HoVer-Net (fp16 / bf16 NHWC activations), HBM-bound:
//   upsample2x_add_act   : out[b, Y, X, :] = act(x[b, Y/2, X/2, :] + y[b, Y, X, :])    half in, half out
//   head 1x1             : y[p][o] = bias[o] + sum_c w[o][c] * pre(x[p][c])            half in, float32 logits out
//   scale_shift_act_view : y = act(x * scale[c] + shift[c]) of a view of a wider buffer  half in, half out
//   grouped_conv_valid   : HoVer-Net's dense-unit Conv2d(128, 32, k, groups=4)           half in, half out, on the 16x16x32 MFMA
//   avgpool2x2 / upsample2x_concat_act : the plain UNet encoder's pooling and the concat skip (kernels in stream_glue.hpp)
// The half forms of tia_upsample2x_add_act_nhwc_f32 / tia_conv1x1_head_nhwc_f32 / tia_scale_shift_act_view_nhwc_f32 /
// tia_grouped_conv_valid_nhwc_f32 (cnn_epilogue.hip).  16 bytes per lane and
// access (8 halves), float32 arithmetic with every step rounded on its own (contraction off: the order of the unfused torch
// ops), ONE round-to-nearest-even to half at the end, 64-bit element offsets (a tensor may exceed 2^31 bytes).
#include "conv_device.hpp"
#include "half_rows.hpp"
#include "stream_glue.hpp"
#include "wide_io.hpp"

#pragma clang fp contract(off)

namespace {

using namespace tia;

constexpr int ET = 256;

// the 16-byte vector of 8 halves as stream_glue.hpp's kernels take it
template <bool BF>
struct HalfVec {
    static constexpr int N = 8;
    static __device__ __forceinline__ void unpack(const v4u& v, float (&f)[8]) { unpack8<BF>(v, f); }
    static __device__ __forceinline__ v4u pack(const float (&f)[8]) { return pack8<BF>(f); }
};

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


// BatchNorm + ReLU of a VIEW (a channel prefix and a spatial window of a wider NHWC half buffer: image / row / pixel strides in
// elements), written densely -- the pre-activations of HoVer-Net's dense units on their in-place feature buffer.  One thread per 8
// channels: p = float(x) * scale; a = p + shift; max(a, 0); one rounding.
template <bool BF>
__global__ __launch_bounds__(ET) void scale_shift_act_view_h_kernel(const unsigned short* __restrict__ x, long sb, long sy, long sp,
                                                                     const float4* __restrict__ scale, const float4* __restrict__ shift,
                                                                     int n, int h, int w, int cv, int relu, v4u* __restrict__ y) {
    const long total = (long)n * h * w * cv;
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < total; i += (long)gridDim.x * ET) {
        const int c = (int)(i % cv);
        long t = i / cv;
        const int px = (int)(t % w);
        t /= w;
        const int py = (int)(t % h), b = (int)(t / h);
        float f[8];
        unpack8<BF>(*reinterpret_cast<const v4u*>(x + (long)b * sb + (long)py * sy + (long)px * sp + 8 * c), f);
        const float4 s0 = scale[2 * c], s1 = scale[2 * c + 1], t0 = shift[2 * c], t1 = shift[2 * c + 1];
        const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
        const float sh[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float v = f[k] * sc[k];
            v = v + sh[k];
            f[k] = relu ? (v > 0.0f ? v : 0.0f) : v;
        }
        y[i] = pack8<BF>(f);
    }
}

// Grouped "valid" K x K convolution, 32 -> 8 channels per group, on v_mfma_f32_16x16x32_f16 / _bf16.  The float32 kernel
// (cnn_epilogue.hip) is a per-thread fmaf chain because a block-diagonal form wasted three quarters of a 32-wide float32 tile; in
// half ONE tap of ONE group is exactly the K = 32 of the 16x16x32 instruction:
//   A (16 rows x 32): the group's weights of the tap, row = output channel (8 real rows, 8 zero rows), lane l holds
//                     A[l & 15][8 (l >> 4) .. + 7] -- kept in registers for all K * K taps (4 VGPRs per tap)
//   B (32 x 16 columns): 16 output pixels, lane l holds channels 8 (l >> 4) .. + 7 of the group of pixel l & 15 under the tap: ONE
//                     16-byte global load, no LDS staging (the 9 / 25 taps of neighbouring pixels re-read lines that sit in L1 / L2)
//   C: column (pixel) l & 15, rows (output channels) 4 (l >> 4) + reg: lanes 0..31 hold the 8 real channels of their pixel; lanes
//      0..15 fetch the upper four from lane + 16 and store the pixel's 8 halves as one 16-byte access
// A wave owns one group and 4 tiles of 16 pixels (the 4 loads of a tap are independent); the 4 waves of a workgroup are 4 groups
// of the same 64 pixels, so together they read whole 256-byte pixels.  float32 accumulation, one rounding; the result may go into a
// channel slice / window of a wider buffer (strides in elements).  No LDS, no barrier.
using f32x4 = __attribute__((ext_vector_type(4))) float;

template <bool BF>
__device__ __forceinline__ f32x4 mma16(const v4u& a, const v4u& b, const f32x4& c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const b8*>(&a), *reinterpret_cast<const b8*>(&b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(&a), *reinterpret_cast<const h8*>(&b), c, 0, 0, 0);
}

constexpr int GC_TILES = 4;  // 16-pixel tiles per wave

template <bool BF, int K>
__global__ __launch_bounds__(ET) void grouped_conv_valid_h_kernel(const unsigned short* __restrict__ x, const v4u* __restrict__ wpk,
                                                                   unsigned short* __restrict__ y, int n, int h, int w, int groups,
                                                                   long y_sb, long y_sy, long y_sp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.y * (ET / 64) + wave;
    if (g >= groups) return;
    const int r = lane & 15, q = lane >> 4;
    const int ho = h - K + 1, wo = w - K + 1;
    const long m_total = (long)n * ho * wo;
    const int cin = groups * 32;
    v4u wr[K * K];
#pragma unroll
    for (int t = 0; t < K * K; ++t) {
        v4u z;
        z.x = z.y = z.z = z.w = 0u;
        wr[t] = r < 8 ? wpk[(((long)g * K * K + t) * 4 + q) * 8 + r] : z;
    }
    const long m0 = (long)blockIdx.x * (16 * GC_TILES);
    const unsigned short* xp[GC_TILES];
    long yo[GC_TILES];
    f32x4 acc[GC_TILES];
#pragma unroll
    for (int t = 0; t < GC_TILES; ++t) {
        const long m = m0 + 16 * t + r;
        const long mm = m < m_total ? m : 0;  // a tile's surplus columns read pixel 0 and store nothing
        const int b = (int)(mm / ((long)ho * wo));
        const int rem = (int)(mm - (long)b * ho * wo);
        const int oy = rem / wo, ox = rem - oy * wo;
        xp[t] = x + (((long)b * h + oy) * w + ox) * cin + g * 32 + 8 * q;
        yo[t] = m < m_total ? (long)b * y_sb + (long)oy * y_sy + (long)ox * y_sp + g * 8 : -1;
        acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            v4u v[GC_TILES];
#pragma unroll
            for (int t = 0; t < GC_TILES; ++t) v[t] = *reinterpret_cast<const v4u*>(xp[t] + ((long)ky * w + kx) * cin);
#pragma unroll
            for (int t = 0; t < GC_TILES; ++t) acc[t] = mma16<BF>(wr[ky * K + kx], v[t], acc[t]);
        }
#pragma unroll
    for (int t = 0; t < GC_TILES; ++t) {
        float o[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[i] = acc[t][i];
            o[4 + i] = __shfl_down(acc[t][i], 16, 64);
        }
        if (q == 0 && yo[t] >= 0) *reinterpret_cast<v4u*>(y + yo[t]) = pack8<BF>(o);
    }
}

// OIHW float32 [groups * 8, 32, k, k] -> [groups][k][k][4 channel chunks][8 outputs][8 halves]: the A operand as the lanes read it
template <bool BF>
__global__ __launch_bounds__(ET) void grouped_pack_h_kernel(const float* __restrict__ w, long total, int k, unsigned short* __restrict__ out) {
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < total; i += (long)gridDim.x * ET) {
        const int j = (int)(i & 7), r = (int)((i >> 3) & 7), q = (int)((i >> 6) & 3);
        const long t = i >> 8;
        const int tap = (int)(t % (k * k));
        const long g = t / (k * k);
        out[i] = f32_to_half<BF>(w[((g * 8 + r) * 32 + 8 * q + j) * (k * k) + tap]);
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

extern "C" int tia_scale_shift_act_view_nhwc_h(const void* d_x, int64_t x_image_stride, int64_t x_row_stride, int64_t x_pixel_stride,
                                               const float* d_scale, const float* d_shift, void* d_y, int64_t n, int64_t h, int64_t w,
                                               int64_t c, int32_t relu, int32_t dtype, void* stream) {
    if (!d_x || !d_scale || !d_shift || !d_y || n <= 0 || h <= 0 || w <= 0 || c <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((c & 7) != 0) return TIA_ESIZE;  // 8 halves per access
    if (((x_image_stride | x_row_stride | x_pixel_stride) & 7) != 0 || x_pixel_stride < c) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_scale) | reinterpret_cast<uintptr_t>(d_shift) |
         reinterpret_cast<uintptr_t>(d_y)) & 15)
        return TIA_EINVAL;
    if (n > 0x7fffffffL || h > 0x7fffffffL || w > 0x7fffffffL) return TIA_ESIZE;
    const long total = n * h * w * (c / 8);
    long blocks = (total + ET - 1) / ET;
    if (blocks > 256L * 64) blocks = 256L * 64;
    const auto kernel = dtype == TIA_DT_BF16 ? scale_shift_act_view_h_kernel<true> : scale_shift_act_view_h_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(ET), 0, (hipStream_t)stream, (const unsigned short*)d_x, (long)x_image_stride,
                       (long)x_row_stride, (long)x_pixel_stride, (const float4*)d_scale, (const float4*)d_shift, (int)n, (int)h, (int)w,
                       (int)(c / 8), relu, (v4u*)d_y);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_grouped_conv_pack_weights_h(const float* d_w_oihw, int64_t groups, int64_t k, int32_t dtype, void* d_packed,
                                               void* stream) {
    if (!d_w_oihw || !d_packed || groups <= 0 || k <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_packed) & 15) return TIA_EINVAL;
    const long total = groups * k * k * 256;
    long blocks = (total + ET - 1) / ET;
    if (blocks > 4096) blocks = 4096;
    const auto kernel = dtype == TIA_DT_BF16 ? grouped_pack_h_kernel<true> : grouped_pack_h_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(ET), 0, (hipStream_t)stream, d_w_oihw, total, (int)k, (unsigned short*)d_packed);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_grouped_conv_valid_nhwc_h(const void* d_x, const void* d_w_packed, void* d_y, int64_t y_image_stride,
                                             int64_t y_row_stride, int64_t y_pixel_stride, int64_t n, int64_t h, int64_t w, int64_t groups,
                                             int64_t cin_per_group, int64_t cout_per_group, int64_t k, int32_t dtype, void* stream) {
    if (!d_x || !d_w_packed || !d_y || n <= 0 || groups <= 0 || groups > 65535 * 4 || k <= 0 || h < k || w < k) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (cin_per_group != 32 || cout_per_group != 8 || (k != 3 && k != 5)) return TIA_ESIZE;  // the taps are unrolled: HoVer-Net's 3 and 5
    if (((y_image_stride | y_row_stride | y_pixel_stride) & 7) != 0 || y_pixel_stride < groups * cout_per_group) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_w_packed) | reinterpret_cast<uintptr_t>(d_y)) & 15) return TIA_EINVAL;
    if (n > 0x7fffffffL || h > 0x7fffffffL || w > 0x7fffffffL || (h - k + 1) * (w - k + 1) > 0x7fffffffL) return TIA_ESIZE;
    const long m_total = n * (h - k + 1) * (w - k + 1);
    const long blocks = (m_total + 16 * GC_TILES - 1) / (16 * GC_TILES);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    using Kernel = void (*)(const unsigned short*, const v4u*, unsigned short*, int, int, int, int, long, long, long);
    const Kernel kernels[2][2] = {{grouped_conv_valid_h_kernel<false, 3>, grouped_conv_valid_h_kernel<false, 5>},
                                  {grouped_conv_valid_h_kernel<true, 3>, grouped_conv_valid_h_kernel<true, 5>}};
    hipLaunchKernelGGL(kernels[dtype == TIA_DT_BF16][k == 5], dim3((unsigned)blocks, (unsigned)((groups + 3) / 4)), dim3(ET), 0,
                       (hipStream_t)stream, (const unsigned short*)d_x, (const v4u*)d_w_packed, (unsigned short*)d_y, (int)n, (int)h, (int)w,
                       (int)groups, (long)y_image_stride, (long)y_row_stride, (long)y_pixel_stride);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_avgpool2x2_nhwc_h(const void* d_x, void* d_y, int64_t n, int64_t h, int64_t w, int64_t c, int32_t dtype, void* stream) {
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (dtype == TIA_DT_BF16) return launch_avgpool2x2<HalfVec<true>>(d_x, d_y, n, h, w, c, (hipStream_t)stream);
    return launch_avgpool2x2<HalfVec<false>>(d_x, d_y, n, h, w, c, (hipStream_t)stream);
}

extern "C" int tia_upsample2x_concat_act_nhwc_h(const void* d_x, const void* d_y, const float* d_scale, const float* d_shift, void* d_out,
                                                int64_t n, int64_t h, int64_t w, int64_t cx, int64_t cy, int32_t dtype, void* stream) {
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (dtype == TIA_DT_BF16)
        return launch_upsample2x_concat<HalfVec<true>>(d_x, d_y, d_scale, d_shift, d_out, n, h, w, cx, cy, (hipStream_t)stream);
    return launch_upsample2x_concat<HalfVec<false>>(d_x, d_y, d_scale, d_shift, d_out, n, h, w, cx, cy, (hipStream_t)stream);
}
