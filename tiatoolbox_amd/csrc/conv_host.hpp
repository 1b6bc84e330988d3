// Host leaves shared by the entry points of the implicit-GEMM convolutions (conv_mfma.hip, conv_mfma_h.hip, conv_ring_bf16x3.hip)
// and, for the batch rule, the Winograd forms (conv3x3_wino.hpp); internal, not part of the C ABI.  The device side of the same
// kernels is conv_device.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tiatoolbox_amd.h"

namespace tia {

// Shape checks of a kh x kw NHWC convolution whose kernel wants cin % cin_multiple == 0 and cout % cout_multiple == 0 (pointer,
// dtype and alignment checks stay with the callers).  Precedence where faults coincide: sizes / positivity TIA_EINVAL, multiples
// TIA_ESIZE, kernel / padding TIA_EINVAL, range TIA_EINVAL.
inline int conv_check_shape(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                            int64_t pad_top, int64_t pad_left, int64_t ho, int64_t wo, int64_t cin_multiple, int64_t cout_multiple) {
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad_top < 0 || pad_left < 0) return TIA_EINVAL;
    if (cin % cin_multiple != 0 || cout % cout_multiple != 0) return TIA_ESIZE;
    // every output pixel must see at least its first tap row / column start inside [-(k-1), h): rows and columns beyond the
    // image on either side read as zeros (that is how asymmetric "same" padding is expressed: pad_top / pad_left + ho / wo)
    if (ho <= 0 || wo <= 0 || kh > 16 || kw > 16 || pad_top >= kh || pad_left >= kw) return TIA_EINVAL;
    if ((ho - 1) * stride - pad_top >= h || (wo - 1) * stride - pad_left >= w) return TIA_EINVAL;
    return TIA_OK;
}

// Images per launch: the kernels address their operands with 32-bit byte offsets, so a batch goes in groups of < 2 GiB of input
// (and < 2^30 output pixels).  0: a single image (or the packed weights) is already too large, or empty.
inline long conv_batch_group(long image_bytes, long w_bytes, long out_pixels) {
    if (image_bytes <= 0 || out_pixels <= 0) return 0;
    if (image_bytes > 0x7fffffffL || w_bytes > 0x7fffffffL || out_pixels > 0x7fffffffL / 4) return 0;
    long group = 0x7fffffffL / image_bytes;
    if (group * out_pixels > 0x7fffffffL / 2) group = 0x7fffffffL / 2 / out_pixels;
    return group;
}

// Grid of the weight packers' grid-stride loops: 256 threads per block, at most 4096 blocks
inline dim3 pack_grid(long total) {
    const long blocks = (total + 255) / 256;
    return dim3((unsigned)(blocks < 4096 ? blocks : 4096));
}

}  // namespace tia
