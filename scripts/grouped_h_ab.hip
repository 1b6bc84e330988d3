// A/B of the two candidate forms of the half-precision grouped valid convolution (HoVer-Net's dense units, 32 -> 8 channels per
// group) at the network's shapes, in one process, alternating:
//   mfma : grouped_conv_valid_h_kernel of csrc/cnn_epilogue_h.hip (one tap of one group = one v_mfma_f32_16x16x32_f16), the form kept
//   dot2 : one thread per output pixel and group (the float32 kernel's shape), 8 float32 accumulators, the pixel's 32 channels as four
//          16-byte loads per tap, the group's weights wave-uniform (scalar loads), v_dot2_f32_f16: 128 packed dots per tap
// Both read the library's packed weights and must agree to float32 summation order.  fp16 only (the question is the form, not the type).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Itiatoolbox_amd/csrc scripts/grouped_h_ab.hip -o grouped_h_ab && ./grouped_h_ab
#include "../tiatoolbox_amd/csrc/cnn_epilogue_h.hip"

#include <cmath>
#include <cstdio>
#include <vector>

namespace {

using half2v = __attribute__((ext_vector_type(2))) _Float16;

template <int K>
__global__ __launch_bounds__(ET) void grouped_dot2_kernel(const unsigned short* __restrict__ x, const v4u* __restrict__ wpk,
                                                           unsigned short* __restrict__ y, int n, int h, int w, int groups) {
    const int g = blockIdx.y;
    const int ho = h - K + 1, wo = w - K + 1;
    const long m_total = (long)n * ho * wo;
    const long m = (long)blockIdx.x * ET + threadIdx.x;
    const long mm = m < m_total ? m : 0;
    const int b = (int)(mm / ((long)ho * wo));
    const int rem = (int)(mm - (long)b * ho * wo);
    const int oy = rem / wo, ox = rem - oy * wo;
    const int cin = groups * 32;
    const unsigned short* xp = x + (((long)b * h + oy) * w + ox) * cin + g * 32;
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int ky = 0; ky < K; ++ky)
        for (int kx = 0; kx < K; ++kx) {
            const v4u* xr = reinterpret_cast<const v4u*>(xp + ((long)ky * w + kx) * cin);
            const v4u* wr = wpk + ((long)g * K * K + ky * K + kx) * 32;  // [chunk 4][output 8] vectors of 8 halves, wave-uniform
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4u v = xr[q];
                const unsigned xv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const v4u wv = wr[q * 8 + r];
                    const unsigned wq[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        acc[r] = __builtin_amdgcn_fdot2(*reinterpret_cast<const half2v*>(&xv[p]), *reinterpret_cast<const half2v*>(&wq[p]), acc[r],
                                                        false);
                }
            }
        }
    if (m < m_total) *reinterpret_cast<v4u*>(y + (((long)b * ho + oy) * wo + ox) * (groups * 8) + g * 8) = pack8<false>(acc);
}

float time_ms(hipStream_t st, int reps, void (*launch)(void*), void* ctx) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    launch(ctx);
    hipEventRecord(e0, st);
    for (int i = 0; i < reps; ++i) launch(ctx);
    hipEventRecord(e1, st);
    hipEventSynchronize(e1);
    float ms = 0.0f;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return ms / reps;
}

struct Case {
    const unsigned short* x;
    const void* wp;
    unsigned short* y;
    int n, side, k;
};

void run_mfma(void* p) {
    const Case& c = *static_cast<Case*>(p);
    const int o = c.side - c.k + 1;
    tia_grouped_conv_valid_nhwc_h(c.x, c.wp, c.y, (long)o * o * 32, (long)o * 32, 32, c.n, c.side, c.side, 4, 32, 8, c.k, TIA_DT_F16, nullptr);
}

void run_dot2(void* p) {
    const Case& c = *static_cast<Case*>(p);
    const int o = c.side - c.k + 1;
    const long m_total = (long)c.n * o * o;
    const dim3 grid((unsigned)((m_total + ET - 1) / ET), 4);
    if (c.k == 3)
        hipLaunchKernelGGL(grouped_dot2_kernel<3>, grid, dim3(ET), 0, nullptr, c.x, (const v4u*)c.wp, c.y, c.n, c.side, c.side, 4);
    else
        hipLaunchKernelGGL(grouped_dot2_kernel<5>, grid, dim3(ET), 0, nullptr, c.x, (const v4u*)c.wp, c.y, c.n, c.side, c.side, 4);
}

}  // namespace

int main() {
    const int n = 32, shapes[3][2] = {{3, 48}, {3, 90}, {5, 60}};
    for (const auto& s : shapes) {
        const int k = s[0], side = s[1], o = side - k + 1;
        const size_t nx = (size_t)n * side * side * 128, ny = (size_t)n * o * o * 32, nw = (size_t)32 * 32 * k * k;
        std::vector<_Float16> hx(nx);
        std::vector<float> hw(nw);
        unsigned seed = 12345u + side;
        auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xffff) / 65536.0f - 0.5f; };
        for (auto& v : hx) v = (_Float16)rnd();
        for (auto& v : hw) v = 0.2f * rnd();
        unsigned short *dx, *dy0, *dy1;
        float* dw;
        void* dwp;
        hipMalloc(&dx, nx * 2), hipMalloc(&dy0, ny * 2), hipMalloc(&dy1, ny * 2), hipMalloc(&dw, nw * 4), hipMalloc(&dwp, nw * 2);
        hipMemcpy(dx, hx.data(), nx * 2, hipMemcpyHostToDevice);
        hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice);
        if (tia_grouped_conv_pack_weights_h(dw, 4, k, TIA_DT_F16, dwp, nullptr) != TIA_OK) return 1;
        Case a{dx, dwp, dy0, n, side, k}, b{dx, dwp, dy1, n, side, k};
        float t_mfma[3], t_dot2[3];
        for (int r = 0; r < 3; ++r) {  // alternating rounds
            t_mfma[r] = time_ms(nullptr, 20, run_mfma, &a);
            t_dot2[r] = time_ms(nullptr, 20, run_dot2, &b);
        }
        if (hipDeviceSynchronize() != hipSuccess) return 2;
        std::vector<_Float16> y0(ny), y1(ny);
        hipMemcpy(y0.data(), dy0, ny * 2, hipMemcpyDeviceToHost);
        hipMemcpy(y1.data(), dy1, ny * 2, hipMemcpyDeviceToHost);
        double dmax = 0.0, vmax = 0.0;
        for (size_t i = 0; i < ny; ++i) {
            dmax = std::fmax(dmax, std::fabs((double)y0[i] - (double)y1[i]));
            vmax = std::fmax(vmax, std::fabs((double)y0[i]));
        }
        auto med = [](float* t) { return t[0] + t[1] + t[2] - std::fmax(t[0], std::fmax(t[1], t[2])) - std::fmin(t[0], std::fmin(t[1], t[2])); };
        const double gb = (nx + ny) * 2 / 1e9;
        std::printf("grouped k%d %dx%dx%dx128->32 fp16: mfma %.4f ms (%.2f TB/s)  dot2 %.4f ms (%.2f TB/s)  dot2/mfma %.2f  max|diff| %.2e of %.2f\n",
                    k, n, side, side, med(t_mfma), gb / med(t_mfma), med(t_dot2), gb / med(t_dot2), med(t_dot2) / med(t_mfma), dmax, vmax);
        hipFree(dx), hipFree(dy0), hipFree(dy1), hipFree(dw), hipFree(dwp);
    }
    return 0;
}
