// Grouped 3x3 convolution, padding 1, stride 1 or 2, float32 NHWC, BN-folded bias and ReLU in the epilogue: the conv2 of the
// ResNeXt Bottleneck (models/architecture/resnet.py: Conv2d(width, width, 3, stride, 1, groups=32)), 4 to 64 channels per group.
//
// One form for every group width, on the vector ALU: gfx950's float32 VALU has the f32 MFMA's peak, and a group of
// 4 or 8 channels is narrower than any f32 MFMA tile.
// * a lane owns P output pixels (m0 + 64 j) of ONE group and OT of its output channels: P x OT accumulators;
// * a wave's group is uniform (wave index through readfirstlane), so the group's weights [tap][c][o] are wave-uniform loads
//   (scalar, from the constant cache): every multiply-add is half of a v_pk_fma_f32 whose weight pair sits in SGPRs;
// * the waves of a workgroup own neighbouring groups of the same pixels, so together they read the pixels' channels
//   contiguously (4 channels x 8 waves, 8 x 4, 16+ x 4 = at least 128 bytes of every pixel);
// * per tap a lane reads its group's CG channels of its P input pixels as 16-byte loads (zero outside the image: padding 1)
//   and issues 4 x OT x P fused multiply-adds per load (2 per v_pk_fma_f32), accumulating in (tap, channel) order.
#include "common.hpp"

namespace tia {

using f2 = __attribute__((ext_vector_type(2))) float;

template <int CG, int OT, int P, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void conv3x3_grouped_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                                      const float* __restrict__ bias, float* __restrict__ y, int n,
                                                                      int h, int w, int ho, int wo, int groups, int stride,
                                                                      int relu) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int g = (int)blockIdx.y * WAVES + wave;
    if (g >= groups) return;  // (wave-uniform; no barrier in this kernel)
    const int o0 = (int)blockIdx.z * OT;
    const int cin = groups * CG;
    const long m_total = (long)n * ho * wo;
    const long m0 = (long)blockIdx.x * (64 * P) + lane;
    int iy0[P], ix0[P];
    bool ok[P];
    const float* xb[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const long m = m0 + 64L * j;
        ok[j] = m < m_total;
        const long mm = ok[j] ? m : 0;
        const int b = (int)(mm / ((long)ho * wo));
        const int rem = (int)(mm - (long)b * ho * wo);
        const int oy = rem / wo, ox = rem - oy * wo;
        iy0[j] = oy * stride - 1;
        ix0[j] = ox * stride - 1;
        xb[j] = x + (long)b * h * w * cin + g * CG;
    }
    f2 acc[P][OT / 2];  // output channel pairs: one v_pk_fma_f32 per pair (input broadcast, two weights from SGPRs)
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int o = 0; o < OT / 2; ++o) acc[j][o] = f2{0.0f, 0.0f};
    const float* wg = wpk + (long)g * 9 * CG * CG + o0;
#pragma unroll 1
    for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t - 3 * (t / 3);
        const float* xp[P];
        bool in[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int iy = iy0[j] + ky, ix = ix0[j] + kx;
            in[j] = ok[j] && iy >= 0 && iy < h && ix >= 0 && ix < w;
            xp[j] = xb[j] + ((long)iy * w + ix) * cin;
        }
        const float* wt = wg + t * CG * CG;
#pragma unroll 8
        for (int c4 = 0; c4 < CG / 4; ++c4) {
            float v[P][4];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (in[j]) f = *reinterpret_cast<const float4*>(xp[j] + 4 * c4);
                v[j][0] = f.x;
                v[j][1] = f.y;
                v[j][2] = f.z;
                v[j][3] = f.w;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f2* wr = reinterpret_cast<const f2*>(wt + (4 * c4 + q) * CG);
#pragma unroll
                for (int o = 0; o < OT / 2; ++o) {
                    const f2 wv = wr[o];
#pragma unroll
                    for (int j = 0; j < P; ++j) acc[j][o] = __builtin_elementwise_fma(f2{v[j][q], v[j][q]}, wv, acc[j][o]);
                }
            }
        }
    }
    const int cout = groups * CG;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        if (!ok[j]) continue;
        float* yp = y + (m0 + 64L * j) * cout + g * CG + o0;
#pragma unroll
        for (int o = 0; o < OT; o += 4) {
            float r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float s = acc[j][(o + i) / 2][(o + i) % 2];
                if (bias) s = s + bias[g * CG + o0 + o + i];
                r[i] = relu ? (s > 0.0f ? s : 0.0f) : s;
            }
            *reinterpret_cast<float4*>(yp + o) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
}

template <int CG, int OT, int P, int WAVES>
static void launch_grouped(const float* x, const float* wpk, const float* bias, float* y, long n, long h, long w, long ho, long wo,
                           long groups, long stride, int relu, hipStream_t st) {
    const long m_total = n * ho * wo;
    const dim3 grid((unsigned)((m_total + 64 * P - 1) / (64 * P)), (unsigned)((groups + WAVES - 1) / WAVES), (unsigned)(CG / OT));
    hipLaunchKernelGGL((conv3x3_grouped_kernel<CG, OT, P, WAVES>), grid, dim3(64 * WAVES), 0, st, x, wpk, bias, y, (int)n, (int)h,
                       (int)w, (int)ho, (int)wo, (int)groups, (int)stride, relu);
}

}  // namespace tia

using namespace tia;

extern "C" int tia_conv3x3_grouped_nhwc_f32(const float* d_x, const float* d_w_packed, const float* d_bias, float* d_y, int64_t n,
                                            int64_t h, int64_t w, int64_t groups, int64_t channels_per_group, int64_t stride,
                                            int32_t relu, void* stream) {
    if (!d_x || !d_w_packed || !d_y || n <= 0 || h <= 0 || w <= 0 || groups <= 0 || (stride != 1 && stride != 2)) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_w_packed) | reinterpret_cast<uintptr_t>(d_y)) & 15)
        return TIA_EINVAL;
    const long cg = channels_per_group;
    if (cg != 4 && cg != 8 && cg != 16 && cg != 32 && cg != 64) return TIA_ESIZE;
    const long ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
    // 32-bit pixel indices in the kernel; the grid's x extent is m_total / (64 P) < 2^31 for any such batch
    if (n * h * w >= (1L << 31) || n * ho * wo >= (1L << 31) || groups > 65535L * 4) return TIA_ESIZE;
    hipStream_t st = (hipStream_t)stream;
    switch (cg) {
        case 4: launch_grouped<4, 4, 4, 8>(d_x, d_w_packed, d_bias, d_y, n, h, w, ho, wo, groups, stride, relu, st); break;
        case 8: launch_grouped<8, 8, 4, 4>(d_x, d_w_packed, d_bias, d_y, n, h, w, ho, wo, groups, stride, relu, st); break;
        case 16: launch_grouped<16, 16, 4, 4>(d_x, d_w_packed, d_bias, d_y, n, h, w, ho, wo, groups, stride, relu, st); break;
        case 32: launch_grouped<32, 32, 2, 4>(d_x, d_w_packed, d_bias, d_y, n, h, w, ho, wo, groups, stride, relu, st); break;
        default: launch_grouped<64, 32, 2, 4>(d_x, d_w_packed, d_bias, d_y, n, h, w, ho, wo, groups, stride, relu, st); break;
    }
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
