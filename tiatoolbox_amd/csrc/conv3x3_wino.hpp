// Internal interface of conv3x3_wino.hip and conv3x3_wino42.hip (not part of the C ABI): the Winograd F(2x2, 3x3) and F(4x2, 3x3)
// float32 convolutions, and the host path and weight-packing tail the two forms share.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.hpp"
#include "conv_device.hpp"
#include "conv_host.hpp"

namespace tia {

// cin % 16 == 0, cout % 64 == 0, front padding 0..2, stride 1 (any map size; maps of at most 8 x 8 go four images per block)
bool conv3x3_wino_serves(long nb, long h, long w, long cin, long cout, long pad_top, long pad_left, long ho, long wo);

// One launch over `nb` images (input extent < 2 GiB: the caller splits the batch).  `u_packed`: tia_conv_pack_weights_wino_f32.
int conv3x3_wino_launch(const float* x, const float* u_packed, const float* bias, const float* residual, float* y, long nb, long h,
                        long w, long cin, long cout, long pad_top, long pad_left, long ho, long wo, int relu, hipStream_t stream);

// Which Winograd form the fused resnet blocks take for a "same"-padded 3x3 / stride-1 layer (conv3x3_wino42.hip): 1 F(4x2), 0 F(2x2)
int conv3x3_wino_form(long n, long h, long w, long cin, long cout, long pad);

// The body of the forms' entry points (tia_conv3x3_wino_nhwc_f32, tia_conv3x3_wino42_nhwc_f32): argument checks, then `launch_group`
// (the signature of conv3x3_wino_launch) once per group of images.  `positions`: Winograd positions of the form (16 | 24), for the
// 32-bit byte offsets into the packed weights.
inline int conv3x3_wino_run(int positions, decltype(&conv3x3_wino_launch) launch_group, const float* d_x, const float* d_u_packed,
                            const float* d_bias, const float* d_residual, float* d_y, long n, long h, long w, long cin, long cout,
                            long pad_top, long pad_left, long ho, long wo, int relu, hipStream_t stream) {
    if (!d_x || !d_u_packed || !d_y || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0) return TIA_EINVAL;
    if (ho <= 0 || wo <= 0 || pad_top < 0 || pad_left < 0 || pad_top > 2 || pad_left > 2) return TIA_EINVAL;
    if (ho - 1 - pad_top >= h || wo - 1 - pad_left >= w) return TIA_EINVAL;  // every output sees at least its first tap row / column start on the map
    if (((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_u_packed) | reinterpret_cast<uintptr_t>(d_y) |
          reinterpret_cast<uintptr_t>(d_residual) | reinterpret_cast<uintptr_t>(d_bias)) & 15) != 0)
        return TIA_EINVAL;
    if (cin % 16 != 0 || cout % 64 != 0) return TIA_ESIZE;
    // 32-bit byte offsets into the input and the packed weights: images go in groups (conv_host.hpp)
    long group = conv_batch_group(h * w * cin * 4, positions * cin * cout * 4, ho * wo);
    if (group < 1) return TIA_ESIZE;
    if (ho <= 8 && wo <= 8 && group > 4) group -= group % 4;  // whole blocks of four images
    if (const long even = even_group(n, group); even < group)
        group = (ho <= 8 && wo <= 8 && even > 4) ? (even + 3) / 4 * 4 : even;  // equal groups (still whole blocks, still <= the limit)
    for (long first = 0; first < n; first += group) {
        const long nb = n - first < group ? n - first : group;
        const int rc = launch_group(d_x + first * h * w * cin, d_u_packed, d_bias, d_residual ? d_residual + first * ho * wo * cout : nullptr,
                                    d_y + first * ho * wo * cout, nb, h, w, cin, cout, pad_top, pad_left, ho, wo, relu, stream);
        if (rc != TIA_OK) return rc;
    }
    return TIA_OK;
}

// Persistent form (one workgroup per CU walks the (pixel block, 64-channel tile) items, the next item's first operands requested
// behind the current one's last steps): an even number of 16-channel slices (the patch buffers alternate per slice and an item must
// end on buffer 1), at least two rounds of items, and a geometry that has the form (`allowed`) -- everything else one block per
// workgroup, blockIdx.x padded to whole rounds of the 8 XCDs.
struct WinoGrid {
    bool persist;
    dim3 grid;
};
inline WinoGrid wino_grid(bool allowed, long tiles, long cin, long cout) {
    static const bool no_persist = dev_env("TIA_WINO_NO_PERSIST") != nullptr;  // developer switch (A/B measurements)
    const long cus = device_cu_count() / 8 * 8;
    const bool persist = !no_persist && allowed && (cin / 16) % 2 == 0 && cus >= 8 && tiles * (cout / 64) >= 2 * cus;
    return WinoGrid{persist, persist ? dim3((unsigned)cus) : dim3((unsigned)(((tiles + 7) / 8) * 8), (unsigned)(cout / 64))};
}

// Launch `Kernel` with `lds` bytes of dynamic LDS beyond the default limit: the attribute that allows it is set once per device.
template <auto Kernel, class... Args>
bool launch_dyn_lds(dim3 grid, dim3 block, int lds, hipStream_t stream, Args... args) {
    static DeviceOnce once;  // (one per kernel)
    if (!once.ensure([lds] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
        }))
        return false;
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return hipGetLastError() == hipSuccess;
}

// Tail of the weight packers, for row i of t = (row transform) g of the (cout o, cin c) pair of a thread: U[i][0..3] = t[i] G2^T
// (G2 = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]) in float64, rounded once, scattered into the stage layout [pos 4 i + j][cin/16][h8 2]
// [cout/64] blocks of 2 KB = [hi 2][64 cout][4 channels] (channel = 16 cs + 8 h8 + 4 hi + c4).
__device__ __forceinline__ void wino_pack_row(const double (&ti)[3], int i, int cout, int cin, int o, int c, float* __restrict__ packed) {
    const int n_cs = cin >> 4, n_cb = cout >> 6;
    const int cs = c >> 4, h8 = (c >> 3) & 1, hi = (c >> 2) & 1, c4 = c & 3, cb = o >> 6, col = o & 63;
    const double uu[4] = {ti[0], 0.5 * (ti[0] + ti[1] + ti[2]), 0.5 * (ti[0] - ti[1] + ti[2]), ti[2]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long block = (((long)(i * 4 + j) * n_cs + cs) * 2 + h8) * n_cb + cb;  // 2 KB = 512 floats
        packed[block * 512 + (hi * 64 + col) * 4 + c4] = (float)uu[j];
    }
}

// The body of the packers' entry points: one thread of `pack_kernel` per (cout, cin) pair
inline int wino_pack_run(int positions, void (*pack_kernel)(const float*, int, int, float*), const float* d_w_oihw, long cout, long cin,
                         float* d_packed, hipStream_t stream) {
    if (!d_w_oihw || !d_packed || cout <= 0 || cin <= 0) return TIA_EINVAL;
    if (cin % 16 != 0 || cout % 64 != 0 || positions * cin * cout * 4 > 0x7fffffffL) return TIA_ESIZE;
    const long total = cout * cin;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, d_w_oihw, (int)cout, (int)cin, d_packed);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

}  // namespace tia
