// Class activation maps of a CNN classifier (models/engine/_cam.py states the quantity; architecture/fused.py: hip_cam):
//   cam[n, k, p] = sum_c w[k, c] * x[n, p, c]      x [n, hw, c] channels-last (float32 | fp16 | bf16), w [k, c] float32, cam float32
// The classifier applied at every position of the trunk's last feature map: no bias, no ReLU, nothing renormalised.
//
// Form.  x is read exactly once and every value meets k multiply-adds (k = 2 .. 32): bandwidth-bound, vector ALU, no MFMA.
//   * One workgroup of 8 waves keeps a tile of `kt` classes of w in LDS ([kt][c] float32, at most 80 KB so that two workgroups share
//     a CU; 9 x 2048 x 4 B = 72 KB is one tile) and sweeps groups of RP = 4 consecutive pixel rows, one group per wave and step.
//   * Lane l owns the 16-byte vectors l, l + 64, ... of a row (4 float32 or 8 halves, widened): one global load per row and vector,
//     one conflict-free ds_read_b128 of w per class and four channels, shared by the four rows (half x: w is stored so that the
//     lanes' quads are consecutive in either half of their 8-channel vectors).
//   * One float32 accumulator per (class, row) and lane: fmaf over the lane's elements in ascending c.  The 64 partial sums of a
//     (class, row) are added in the butterfly order v[l] + v[l ^ 32], then ^ 16, 8, 4, 2, 1; the first four steps exchange halves of
//     the accumulator set instead of every accumulator (each lane sends what its partner keeps), which is the same additions on a
//     twelfth of the exchanges.  That order depends on c alone: not on the row's place in its group, the batch or the grid, so a
//     patch gives the same bits in any batch.
//   * No atomics, no scratch.  More classes than a tile holds: the sweep repeats per tile (x is then read once per tile).
// 64-bit element offsets.
#include "half_rows.hpp"

namespace {

using namespace tia;

using f4 = __attribute__((ext_vector_type(4))) float;

constexpr int CT = 768;                  // threads per workgroup (12 waves: three per SIMD, 168 registers each)
constexpr int KT = 12;                   // classes per tile at most (kernel forms of 4, 8 and 12): KQ * RP accumulators per lane
constexpr int RP = 4;                    // pixel rows per wave and step
constexpr int kLdsBudget = 144 * 1024;   // bytes of w per workgroup: one workgroup per CU
constexpr int kMaxC = 8192;              // kLdsBudget / (4 * kMaxC) >= 1 class per tile
constexpr int kMaxBlocks = 256;          // one per CU

// elements 4 h .. 4 h + 3 of a 16-byte vector of x, widened to float32
template <int DT>
__device__ __forceinline__ void widen4(const v4u& v, int h, float (&f)[4]) {
    if constexpr (DT == TIA_DT_F32) {
        f[0] = __uint_as_float(v.x), f[1] = __uint_as_float(v.y), f[2] = __uint_as_float(v.z), f[3] = __uint_as_float(v.w);
    } else {
        const unsigned lo = h == 0 ? v.x : v.z, hi = h == 0 ? v.y : v.w;
        f[0] = half_to_f32<DT == TIA_DT_BF16>((unsigned short)(lo & 0xffffu));
        f[1] = half_to_f32<DT == TIA_DT_BF16>((unsigned short)(lo >> 16));
        f[2] = half_to_f32<DT == TIA_DT_BF16>((unsigned short)(hi & 0xffffu));
        f[3] = half_to_f32<DT == TIA_DT_BF16>((unsigned short)(hi >> 16));
    }
}

// KQ: the accumulator rows of this form.  A tile of kn < KQ classes leaves rows kn .. KQ - 1 to repeat class kn - 1 (no branch in the
// loop; they are not stored).
template <int DT, int KQ>
__global__ __launch_bounds__(CT) void cam_nhwc_kernel(const v4u* __restrict__ x, const float* __restrict__ w, float* __restrict__ out,
                                                      long rows, int hw, int c, int k, int kt) {
    // [kt][c] float32 as 16-byte quads.  float32 x: in channel order.  Half x, where a lane's vector is 8 channels: inside every block
    // of 64 vectors the 64 first quads, then the 64 second quads, so that the lanes of a wave read consecutive quads in either half
    // of their vectors (in channel order they would be 32 bytes apart: a bank conflict on every read).
    extern __shared__ f4 wl[];
    constexpr int VE = DT == TIA_DT_F32 ? 4 : 8;  // elements per 16-byte vector of x
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = c / VE, cq = c / 4;
    const long groups = (rows + RP - 1) / RP;
    for (int k0 = 0; k0 < k; k0 += kt) {
        const int kn = k - k0 < kt ? k - k0 : kt;
        __syncthreads();  // (the tile before this one has been read by every wave)
        for (int i = threadIdx.x; i < kn * cq; i += CT) {
            int at = i;
            if constexpr (VE == 8) {
                const int q = i / cq, j = i - q * cq, v = j >> 1, blk = v & ~63, lanes = nv - blk < 64 ? nv - blk : 64;
                at = q * cq + 2 * blk + (j & 1) * lanes + (v & 63);
            }
            wl[at] = reinterpret_cast<const f4*>(w + (long)k0 * c)[i];
        }
        __syncthreads();
        for (long g = (long)blockIdx.x * (CT / 64) + wave; g < groups; g += (long)gridDim.x * (CT / 64)) {
            const long r0 = g * RP;
            const v4u* xr[RP];
#pragma unroll
            for (int i = 0; i < RP; ++i) {
                const long r = r0 + i < rows ? r0 + i : rows - 1;  // (a row past the end reads the last one and is not stored)
                xr[i] = x + r * nv;
            }
            float acc[KQ * RP];
#pragma unroll
            for (int i = 0; i < KQ * RP; ++i) acc[i] = 0.0f;
            for (int v = lane; v < nv; v += 64) {
                v4u xv[RP];
#pragma unroll
                for (int i = 0; i < RP; ++i) xv[i] = xr[i][v];
                // this lane's first quad of w within a class row, and the distance to its second (half x: the layout above)
                const int lanes = VE == 8 ? (nv - (v - lane) < 64 ? nv - (v - lane) : 64) : 0;
                const int at0 = VE == 8 ? 2 * (v - lane) + lane : v;
#pragma unroll 1  // (unrolled, the reads of w for both halves of a vector are hoisted together and the registers run out)
                for (int h = 0; h < VE / 4; ++h) {  // four elements at a time: the halves are widened once, not once per class
                    float xf[RP][4];
#pragma unroll
                    for (int i = 0; i < RP; ++i) widen4<DT>(xv[i], h, xf[i]);
#pragma unroll
                    for (int q = 0; q < KQ; ++q) {
                            const f4 t = wl[(q < kn ? q : kn - 1) * cq + at0 + h * lanes];
                            const float wf[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                            for (int i = 0; i < RP; ++i)
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc[q * RP + i] = fmaf(xf[i][e], wf[e], acc[q * RP + i]);
                    }
                }
            }
            // the butterfly over the wave.  Steps 32, 16, 8, 4: a lane keeps the half of the set that its bit names and sends the
            // other half, so that after them lane l holds the sums of the T = KQ * RP / 16 accumulators
            // T (8 b5 + 4 b4 + 2 b3 + b2) + {0 .. T - 1} over the lanes that differ from it in those bits; steps 2 and 1 fold these in full.
            constexpr int T = KQ * RP / 16;
            static_assert(KQ * RP % 16 == 0 && T <= 4, "the exchange leaves T accumulators per lane, stored by the lanes of a quad");
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int mask = 32 >> s, half = (KQ * RP) >> (s + 1);
                const bool hi = (lane & mask) != 0;
#pragma unroll
                for (int i = 0; i < half; ++i) {
                    const float a = acc[i], b = acc[i + half];
                    acc[i] = (hi ? b : a) + __shfl_xor(hi ? a : b, mask, 64);
                }
            }
            float val = 0.0f;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                acc[t] += __shfl_xor(acc[t], 2, 64);
                acc[t] += __shfl_xor(acc[t], 1, 64);
                val = (lane & 3) == t ? acc[t] : val;
            }
            const int idx = T * (lane >> 2) + (lane & 3);
            const int q = idx / RP;
            const long r = r0 + idx % RP;
            if ((lane & 3) < T && q < kn && r < rows) out[(r / hw) * ((long)k * hw) + (long)(k0 + q) * hw + r % hw] = val;
        }
    }
}

DeviceOnce g_cam_once[3][3];

template <int DT>
int launch_cam(const void* x, const float* w, float* out, int64_t n, int hw, int c, int k, hipStream_t st) {
    if (!x || !w || !out || n <= 0 || hw <= 0 || c <= 0 || k <= 0) return TIA_EINVAL;
    if ((c & 63) != 0 || c > kMaxC) return TIA_ESIZE;
    if (n > 0x7fffffffL || (long)hw * k > 0x7fffffffL) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w)) & 15) return TIA_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) & 3) return TIA_EINVAL;
    int kt = kLdsBudget / (4 * c);
    kt = kt > KT ? KT : kt;
    kt = kt > k ? k : kt;
    const int lds = kt * c * 4;
    const long rows = (long)n * hw, groups = (rows + RP - 1) / RP;
    long blocks = (groups + CT / 64 - 1) / (CT / 64);
    blocks = blocks > kMaxBlocks ? kMaxBlocks : blocks;
    auto launch = [&](auto kernel, DeviceOnce& once) {
        if (!once.ensure([&] {
                return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget) ==
                       hipSuccess;
            }))
            return TIA_ELAUNCH;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CT), lds, st, static_cast<const v4u*>(x), w, out, rows, hw, c, k, kt);
        return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
    };
    if (kt <= 4) return launch(cam_nhwc_kernel<DT, 4>, g_cam_once[DT][0]);
    if (kt <= 8) return launch(cam_nhwc_kernel<DT, 8>, g_cam_once[DT][1]);
    return launch(cam_nhwc_kernel<DT, KT>, g_cam_once[DT][2]);
}

}  // namespace

extern "C" int tia_cam_nhwc_f32(const float* d_x, const float* d_w, float* d_out, int64_t n, int32_t hw, int32_t c, int32_t k, void* stream) {
    return launch_cam<TIA_DT_F32>(d_x, d_w, d_out, n, hw, c, k, (hipStream_t)stream);
}

extern "C" int tia_cam_nhwc_h(const void* d_x, const float* d_w, float* d_out, int64_t n, int32_t hw, int32_t c, int32_t k, int32_t dtype,
                              void* stream) {
    if (dtype == TIA_DT_F16) return launch_cam<TIA_DT_F16>(d_x, d_w, d_out, n, hw, c, k, (hipStream_t)stream);
    if (dtype == TIA_DT_BF16) return launch_cam<TIA_DT_BF16>(d_x, d_w, d_out, n, hw, c, k, (hipStream_t)stream);
    return TIA_EINVAL;
}
