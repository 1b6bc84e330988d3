// kh x kw NHWC float32 convolution (any stride; the strided 3x3 convolutions of torchvision's BasicBlock / Bottleneck behind
// CNNModel.forward, models/architecture/vanilla.py:300-316) on the gfx950 BF16 matrix cores with BOTH operands split into three bf16
// numbers: float32 in, float32 accumulate, another summation order than the float32 ring kernel (conv1x1_ring_kernel,
// conv3x3_spatial.hip), bias + residual + ReLU fused.  DESIGN 4.27.
//
// Arithmetic.  A float32 number is exactly the sum of three bf16 numbers, v = hi + mid + lo with hi = bf16(v), mid = bf16(v - hi),
// lo = bf16(v - hi - mid) (round to nearest even; both subtractions are exact in float32), so a * w = sum_ij a_i * w_j is an
// identity of nine terms, each a product of two 8-bit significands and therefore exact in the float32 accumulator of
// v_mfma_f32_32x32x16_bf16.  Six terms carry everything float32 can see; mid * lo, lo * mid and lo * lo are dropped (together
// below 2^-23 |a w|).  v_mfma_f32_32x32x16_bf16 does K = 16 in 32 cycles where v_mfma_f32_32x32x2_f32 does K = 2 in 64: six of
// them per 16 channels are 192 matrix-pipe cycles against 512.
//   * per 16-channel slice and 32 x 32 tile six MFMAs go into ONE accumulator, smallest terms first (activation part x weight part):
//     lo * hi, hi * lo, mid * mid, mid * hi, hi * mid, hi * hi
//   * the weights are split once, at pack time (fused.split_stem_weights + tia_conv_pack_weights_bf16x3); the activations are split
//     in registers: a lane of the bf16 MFMA holds row lane & 31, k = 8 (lane >> 5) .. + 7 -- the same eight float32 channels the
//     float32 kernel's lane reads with two ds_read_b128.  Per pair of values: v_cvt_pk_bf16_f32, two unpacks (shift / mask), two
//     v_sub_f32, and again, and a third v_cvt_pk_bf16_f32: 44 vector instructions per 32 x 16 fragment.  (The truncating form --
//     v_and_b32 0xffff0000 / v_sub_f32 / v_perm_b32 -- is an exact split as well and costs the same count; it keeps huge inputs
//     finite where this one overflows, see below.  Rounding is what the weights use and what the tests pin.)
//
// Machinery: the ring kernel's.  A workgroup of 512 threads owns 256 consecutive output pixels x 128 output channels; the reduction
// runs over (tap row, tap column, 16-channel slice); both operands arrive by LDS-DMA into the idle one of two stages while the
// waves work on the other (one barrier and one vmcnt(0) per slice); a padding tap is an out-of-range offset (the DMA writes zeros).
//   * A stage: raw float32, pixel pitch 5 units of 16 bytes (the bank argument of conv3x3_spatial.hip): 20 KB
//   * B stage: [3 planes][2 k-chunks][128 columns][8 bf16] = 12 KB, CONTIGUOUS in the packed weights ([tap][cin/16][cout/128] stages):
//     a lane's eight k values of a column are one conflict-free ds_read_b128 per plane and column tile
//   * waves: 8 along the pixels x 1: a wave owns 32 pixels x 128 channels = four accumulator tiles (64 registers), splits ONE
//     A fragment per slice (44 + 2 reads) and reads 12 weight fragments beside its 24 MFMAs (768 pipe cycles) -- the 4 x 2 layout of the
//     float32 kernel would split every A fragment twice
//   * two stages of 32 KB; the epilogue's 64 KB tile aliases them: two workgroups per CU
//   * epilogue through the LDS tile in two column halves: + bias + residual, ReLU, 16-byte stores; XCD-contiguous block order
//
// Invalid-input domain.  A non-finite activation, or one with |a| >= 2^127 (2 - 2^-8) = 3.3961e38 (hi rounds to infinity,
// v - hi = -inf, the third part NaN), makes every output that reads it non-finite: never a finite wrong value.  (Below that
// boundary hi is at most the largest bf16 number 2^127 (2 - 2^-7) and the split is exact.)  Parts below the bf16 normal
// range (|part| < 2^-126) may be flushed to zero by the matrix cores: an absolute error of at most 2^-126 |w| per product.
// The weights' parts are checked on the host (a split that is not exact and normal is not packed: pack_conv_weights_split).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/tiatoolbox_amd.h"
#include "common.hpp"
#include "conv_device.hpp"
#include "conv_host.hpp"
#include "dev_env.hpp"

namespace {

using namespace tia;

// Phase timing (developer builds only: -DTIA_SPLIT_TIMING=1, build.build(defines=...)): thread 0 of two workgroups prints the
// shader-clock cycles of set-up, first-data wait, slice loop and epilogue, and the sustained shader clock (against the constant
// 100 MHz clock), in the manner of TIA_SP_TIMING.
#ifndef TIA_SPLIT_TIMING
#define TIA_SPLIT_TIMING 0
#endif
#if TIA_SPLIT_TIMING
#define SSTAMP(i) { const long long now_ = clock64(); tm_[i] = now_ - tl_; tl_ = now_; }
#else
#define SSTAMP(i)
#endif

template <int BN>
__global__ __launch_bounds__(512, 4) void conv_ring_bf16x3_kernel(const float* __restrict__ x, const void* __restrict__ wk,
                                                                 const float* __restrict__ bias, const float* __restrict__ res,
                                                                 float* __restrict__ y, PwDims d, int relu, int m_tiles) {
    static_assert(BN == 128, "a weight stage is [3][2][128][8]");
    constexpr int NT = 512, NTILE = BN / 32, PIX = 5;
    constexpr int A_UNITS = 256 * PIX;   // 1280 units: two whole DMA rounds of 512 + 256
    constexpr int A_BYTES = A_UNITS * 16;
    constexpr int B_UNITS = 3 * 2 * BN;  // 768 units: one whole DMA round + 256
    constexpr int B_BYTES = B_UNITS * 16;
    constexpr int STAGE = A_BYTES + B_BYTES;
    constexpr int DUMP = 2 * STAGE;      // 1 KB that the idle waves of the partial DMA rounds write their zeros to
    constexpr int EPI = 256 * (BN / 2) * 4;
    constexpr int LDS_BYTES = (DUMP + 1024) > EPI ? (DUMP + 1024) : EPI;
    static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];

#if TIA_SPLIT_TIMING
    long long tm_[4] = {0, 0, 0, 0}, tl_ = clock64();
    const long long t0c_ = tl_, t0w_ = wall_clock64();
#endif
    const int mt_id = xcd_tile(blockIdx.x, m_tiles);
    if (mt_id >= m_tiles) return;
    const long m0 = (long)mt_id * 256;
    const long m_total = (long)d.n * d.ho * d.wo;
    const int n0 = blockIdx.y * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)d.x_bytes, kBufferRsrcFlags);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(wk), 0, (int)d.w_bytes, kBufferRsrcFlags);

    // per DMA unit: byte offset of tap (0, 0) of its pixel (may lie before the buffer: only used when the tap is inside the image)
    // and one bit per kernel row / column saying whether that row / column of taps is inside (all set for a 1x1)
    int cen[3];
    unsigned msk[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int u = NT * r + tid;
        const int p = u / PIX, chunk = u - p * PIX;
        const long m = m0 + p;
        const bool ok = p < 256 && chunk < 4 && m < m_total;
        const int mm = ok ? (int)m : 0;
        const int b = mm / (d.ho * d.wo), rem = mm - b * d.ho * d.wo;
        const int oy = rem / d.wo, ox = rem - oy * d.wo;
        const int iy0 = oy * d.stride - d.pad_y, ix0 = ox * d.stride - d.pad_x;
        cen[r] = (((b * d.h + iy0) * d.w + ix0) * d.cin) * 4 + 16 * chunk;
        unsigned rows = 0, cols = 0;
        for (int t = 0; t < d.kh; ++t) rows |= (unsigned)((unsigned)(iy0 + t) < (unsigned)d.h) << t;
        for (int t = 0; t < d.kw; ++t) cols |= (unsigned)((unsigned)(ix0 + t) < (unsigned)d.w) << (16 + t);
        msk[r] = ok ? (rows | cols) : 0u;
    }
    // weight stage: unit NT r + tid of the 768 (the second round is the lower four waves')
    const int b_off1 = tid < B_UNITS - NT ? (NT + tid) * 16 : OOB;
    const int n_cs = d.cin >> 4;
    const int n_slices = d.kh * d.kw * n_cs;
    const int col_tiles = d.cout / BN;

    // slice cursor: s.c counts 16-channel slices; past the last slice the idle stage is refilled with the same slice
    SliceCursor s;
    auto dma_stage = [&](int stage) {
        unsigned char* sa = smem + stage * STAGE;
        const int sdelta = (s.kh * d.w + s.kw) * d.cin * 4;
        const unsigned sel = (1u << s.kh) | (1u << (16 + s.kw));
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            unsigned char* dst = (NT * r + wave * 64 >= A_UNITS) ? smem + DUMP : sa + r * (NT * 16) + wave * 1024;
            dma16(rx, dst, (msk[r] & sel) == sel ? cen[r] + sdelta : OOB, s.c * 64);
        }
        const int wstage = ((((s.kh * d.kw + s.kw) * n_cs) + s.c) * col_tiles + (int)blockIdx.y) * B_BYTES;
        dma16(rw, sa + A_BYTES + wave * 1024, tid * 16, wstage);
        dma16(rw, (NT + wave * 64 >= B_UNITS) ? smem + DUMP : sa + A_BYTES + NT * 16 + wave * 1024, b_off1, wstage);
    };

    f32x16 acc[NTILE];
#pragma unroll
    for (int j = 0; j < NTILE; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;

    const int hi = lane >> 5;
    const int fa0 = (wave * 32 + (lane & 31)) * PIX + 2 * hi;  // MFMA row = pixel wave * 32 + (lane & 31); channels 8 hi .. 8 hi + 7
    const int fb0 = hi * BN + (lane & 31);                     // plane 0, k-chunk hi, column lane & 31 of tile 0

    dma_stage(0);
    SSTAMP(0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    SSTAMP(1)
    for (int it = 0; it < n_slices; ++it) {
        const int stage = it & 1;
        s.next(1, n_cs, d.kh, d.kw);
        dma_stage(stage ^ 1);
        const u32x4* sa = reinterpret_cast<const u32x4*>(smem + stage * STAGE) + fa0;
        const u32x4* sb = reinterpret_cast<const u32x4*>(smem + stage * STAGE + A_BYTES) + fb0;
        const u32x4 a0 = sa[0], a1 = sa[1];
        u32x4 ah, am, al;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // packed register q = channels 8 hi + 2 q, + 1
            const u32x4& src = q < 2 ? a0 : a1;
            unsigned ph, pm, pl;
            split_pair(__uint_as_float(src[2 * (q & 1)]), __uint_as_float(src[2 * (q & 1) + 1]), ph, pm, pl);
            ah[q] = ph, am[q] = pm, al[q] = pl;
        }
#pragma unroll
        for (int j = 0; j < NTILE; ++j) {
            const u32x4 bh = sb[j * 32], bm = sb[2 * BN + j * 32], bl = sb[4 * BN + j * 32];
            acc[j] = mfma_bf16(al, bh, acc[j]);
            acc[j] = mfma_bf16(ah, bl, acc[j]);
            acc[j] = mfma_bf16(am, bm, acc[j]);
            acc[j] = mfma_bf16(am, bh, acc[j]);
            acc[j] = mfma_bf16(ah, bm, acc[j]);
            acc[j] = mfma_bf16(ah, bh, acc[j]);
        }
        __builtin_amdgcn_sched_barrier(0);  // the slice's MFMAs are issued HERE, in front of the wait: they are the DMA's cover
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    SSTAMP(2)
    __syncthreads();

    // epilogue: per column half (tiles 2 half, 2 half + 1 of every wave): accumulators -> float32 LDS tile [256][64], then every
    // thread takes rows x 8-column chunks: + bias + residual, ReLU, 16-byte stores
    constexpr int HB = BN / 2, CHUNKS = 256 * HB / 8;
    float* tile = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int jj = 0; jj < NTILE / 2; ++jj)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                tile[row * HB + jj * 32 + (lane & 31)] = acc[half * (NTILE / 2) + jj][e];
            }
        __syncthreads();
        for (int idx = tid; idx < CHUNKS; idx += NT) {
            const int row = idx / (HB / 8), cc = idx - row * (HB / 8);
            const long m = m0 + row;
            if (m < m_total) {
                const int col0 = n0 + half * HB + cc * 8;
                const float4 v0 = *reinterpret_cast<const float4*>(tile + row * HB + cc * 8);
                const float4 v1 = *reinterpret_cast<const float4*>(tile + row * HB + cc * 8 + 4);
                float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                if (bias) {
                    const float4 b0 = *reinterpret_cast<const float4*>(bias + col0), b1 = *reinterpret_cast<const float4*>(bias + col0 + 4);
                    v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
                    v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
                }
                float* yo = y + m * d.cout + col0;
                if (res) {
                    const float* rp = res + m * d.cout + col0;
                    const float4 r0 = *reinterpret_cast<const float4*>(rp), r1 = *reinterpret_cast<const float4*>(rp + 4);
                    v[0] += r0.x; v[1] += r0.y; v[2] += r0.z; v[3] += r0.w;
                    v[4] += r1.x; v[5] += r1.y; v[6] += r1.z; v[7] += r1.w;
                }
                if (relu) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = v[k] > 0.0f ? v[k] : 0.0f;
                }
                *reinterpret_cast<float4*>(yo) = float4{v[0], v[1], v[2], v[3]};
                *reinterpret_cast<float4*>(yo + 4) = float4{v[4], v[5], v[6], v[7]};
            }
        }
        __syncthreads();
    }
#if TIA_SPLIT_TIMING
    SSTAMP(3)
    // two workgroups report: an early one (of the first wave of workgroups) and one three quarters through the grid, both on XCD 0
    // (a multiple of 8 is pixel tile bid / 8 < m_tiles, so neither has left at the top)
    const int early_ = gridDim.x > 64 ? 64 : 0, late_ = 8 * (3 * xcd_share(m_tiles) / 4);
    if (threadIdx.x == 0 && blockIdx.y == 0 && ((int)blockIdx.x == early_ || (int)blockIdx.x == late_))
        printf("split ring wg %d (cin %d, %d x %d taps): setup %lld  first-data wait %lld  slice loop %lld  epilogue %lld  | shader clock %.0f MHz\n",
               (int)blockIdx.x, d.cin, d.kh, d.kw, tm_[0], tm_[1], tm_[2], tm_[3],
               100.0 * (double)(clock64() - t0c_) / (double)(wall_clock64() - t0w_));
#endif
}

// parts [3][cout][cin][kh][kw] float32 (bf16 values) -> [kh][kw][cin/16][cout/128][3][2][128][8] bf16: the stage of (tap, slice cs,
// column tile ct) holds, for plane p, k-chunk q, column c and element e, part p of w[128 ct + c][16 cs + 8 q + e][tap]
__global__ __launch_bounds__(256) void pack_bf16x3_kernel(const float* __restrict__ parts, int cout, int cin, int kh, int kw,
                                                          unsigned short* __restrict__ out) {
    const long total = 3L * cout * cin * kh * kw;
    const int n_cs = cin >> 4, col_tiles = cout >> 7;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int e = (int)(i & 7), c = (int)((i >> 3) & 127), q = (int)((i >> 10) & 1);
        long t = i >> 11;
        const int p = (int)(t % 3);
        t /= 3;
        const int ct = (int)(t % col_tiles);
        t /= col_tiles;
        const int cs = (int)(t % n_cs);
        t /= n_cs;
        const int tx = (int)(t % kw), ty = (int)(t / kw);
        const long o = 128L * ct + c, ch = 16L * cs + 8 * q + e;
        const float v = parts[((((long)p * cout + o) * cin + ch) * kh + ty) * kw + tx];
        out[i] = (unsigned short)(__float_as_uint(v) >> 16);  // a bf16 value by contract: the low half is zero
    }
}

}  // namespace

extern "C" int tia_conv_pack_weights_bf16x3(const float* d_parts_oihw, int64_t cout, int64_t cin, int64_t kh, int64_t kw, void* d_packed,
                                            void* stream) {
    if (!d_parts_oihw || !d_packed || cout <= 0 || cin <= 0 || kh <= 0 || kw <= 0) return TIA_EINVAL;
    if (cin % 16 != 0 || cout % 128 != 0) return TIA_ESIZE;
    const long total = 3L * cout * cin * kh * kw;
    hipLaunchKernelGGL(pack_bf16x3_kernel, tia::pack_grid(total), dim3(256), 0, (hipStream_t)stream, d_parts_oihw, (int)cout, (int)cin,
                       (int)kh, (int)kw, static_cast<unsigned short*>(d_packed));
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_conv2d_bf16x3_nhwc_f32(const float* d_x, const void* d_w_packed3, const float* d_bias, const float* d_residual,
                                          float* d_y, int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh,
                                          int64_t kw, int64_t stride, int64_t pad_top, int64_t pad_left, int32_t relu, void* stream) {
    if (!d_x || !d_w_packed3 || !d_y) return TIA_EINVAL;
    if (h <= 0 || w <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad_top < 0 || pad_left < 0) return TIA_EINVAL;
    // symmetric padding (pad_top rows behind as in front), as tia_conv2d_nhwc_f32
    const long ho = (h + 2 * pad_top - kh) / stride + 1, wo = (w + 2 * pad_left - kw) / stride + 1;
    // the argument checks of the float32 entry (conv2d_impl, conv_mfma.hip) with this kernel's multiples: cin % 16, cout % 128
    if (const int rc = tia::conv_check_shape(n, h, w, cin, cout, kh, kw, stride, pad_top, pad_left, ho, wo, 16, 128); rc != TIA_OK) return rc;
    if (((reinterpret_cast<uintptr_t>(d_w_packed3) | reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y) |
          reinterpret_cast<uintptr_t>(d_bias) | reinterpret_cast<uintptr_t>(d_residual)) & 15) != 0)
        return TIA_EINVAL;
    const long image_bytes = h * w * cin * 4, w_bytes = kh * kw * cin * cout * 6;
    const long group = tia::even_group(n, tia::conv_batch_group(image_bytes, w_bytes, ho * wo));
    if (group < 1) return TIA_ESIZE;
    for (long first = 0; first < n; first += group) {
        const long nb = n - first < group ? n - first : group;
        const long tiles = (nb * ho * wo + 255) / 256;
        const PwDims d{(int)nb, (int)h, (int)w, (int)cin, (int)cout, (int)ho, (int)wo, (int)stride, (unsigned)(nb * image_bytes),
                       (unsigned)w_bytes, (int)kh, (int)kw, (int)pad_top, (int)pad_left};
        const dim3 grid((unsigned)(((tiles + 7) / 8) * 8), (unsigned)(cout / 128));
        hipLaunchKernelGGL(conv_ring_bf16x3_kernel<128>, grid, dim3(512), 0, (hipStream_t)stream, d_x + first * h * w * cin, d_w_packed3,
                           d_bias, d_residual ? d_residual + first * ho * wo * cout : nullptr, d_y + first * ho * wo * cout, d, relu,
                           (int)tiles);
    }
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

// Where conv_algo="auto" takes the split kernel (host only, no device needed).  Two conditions:
//   1. the float32 entry would run the shape on the LDS-DMA ring (tia_conv2d_route_f32 == 2: same tile, same grid, same fill rule;
//      small launches stay on the slice kernel), and
//   2. the layer class measured faster than the float32 ring kernel by more than the run-to-run spread of three interleaved rounds.
// Measured (scripts/perf_conv_split.py, profiles/conv_split_perf.txt; 4096 patches; float32 ring -> split, ms; spread of the rounds in
// brackets): the strided layers of ResNet layers 2-4, at both map sizes
//     K = kh kw cin   256^2 patches                          224^2 patches
//   3x3 / 2   576     4.95 -> 3.17  x1.56  [0.3 / 1.1 %]     3.75 -> 2.41  x1.56  [0.1 / 0.8 %]
//   3x3 / 2  1152     4.64 -> 3.00  x1.55  [1.3 / 0.1 %]     3.62 -> 2.29  x1.58  [1.4 / 0.9 %]
//   3x3 / 2  2304     4.55 -> 2.94  x1.55  [2.0 / 0.6 %]     3.74 -> 2.30  x1.62  [0.2 / 1.4 %]
//   1x1 / 2    64     0.90 -> 0.74  x1.21  [4.3 / 2.0 %]     0.69 -> 0.57  x1.20  [4.3 / 0.8 %]
//   1x1 / 2   128     0.69 -> 0.53  x1.30  [2.0 / 0.6 %]     0.54 -> 0.41  x1.32  [2.7 / 0.7 %]
//   1x1 / 2   256     0.60 -> 0.41  x1.44  [4.3 / 0.2 %]     0.49 -> 0.32  x1.54  [1.7 / 0.1 %]
// Every measured class gains more than its spread, the smallest (K = 64) 20 % against 4 %.  RULE: stride 2 (the class measured) and
// K = kh kw cin >= 64 (the smallest K measured).  Stride-1 shapes on the ring (1x1 of Bottleneck trunks) were not measured and stay.
// Developer switch (TIA_DEV=1): TIA_CONV_NO_SPLIT makes the answer 0 (A/B runs from one build).
extern "C" int tia_conv2d_bf16x3_serves(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t kh, int64_t kw, int64_t stride,
                                        int64_t pad_top, int64_t pad_left, int64_t ho, int64_t wo) {
    static const bool disabled = tia::dev_env("TIA_CONV_NO_SPLIT") != nullptr;
    if (disabled) return 0;
    if (tia::conv_check_shape(n, h, w, cin, cout, kh, kw, stride, pad_top, pad_left, ho, wo, 16, 128) != TIA_OK) return 0;
    if (tia_conv2d_route_f32(n, h, w, cin, cout, kh, kw, stride, pad_top, pad_left, ho, wo) != 2) return 0;
    // the entry point pads symmetrically: the output size must be the one it derives
    if (ho != (h + 2 * pad_top - kh) / stride + 1 || wo != (w + 2 * pad_left - kw) / stride + 1) return 0;
    constexpr long kSplitMinK = 64;
    return stride == 2 && kh * kw * cin >= kSplitMinK ? 1 : 0;
}
