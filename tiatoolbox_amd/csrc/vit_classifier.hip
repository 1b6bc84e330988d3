// The two ends of a Vision Transformer classifier (models/architecture/vit_fused.py: FusedViT.forward_uint8, FusedViTClassifier):
//   vit_patchify_norm_u8 : uint8 NHWC patches -> [n, g, k_pad] half tokens, every byte replaced by its entry of a [256][3] table
//                          (ToTensor + Normalize(mean, std), worked out once on the host) -- a gather, no arithmetic
//   linear_softmax_rows  : p[r, :] = softmax(x[r, :f] . W^T + b) on the graph's float32 features, float32 throughout
// 64-bit element offsets; nothing here depends on the grid, so a row's (a patch's) result is the same in any batch.
#include "half_rows.hpp"
#include "wide_io.hpp"

namespace {

using namespace tia;

constexpr int ET = 256;

// One thread per 8 output halves of a k_pad-wide token row, as in vit_patchify_pad_h_kernel: columns (ky, kx, c), zeros from 3 p^2 on,
// one aligned 16-byte store.
//
// The table.  `lut` is d_table as it is, [256][3] halves (6 bytes per byte value).  The 8 values of a thread are 8 consecutive bytes
// of a patch row, i.e. channels c0, c0 + 1, ... in turn, and neighbouring lanes start 8 bytes apart: ONE ds_read_u16 of the wave mixes
// all three channels.  Slide background is grey (R = G = B) and tissue is smooth, so the lanes of a read mostly hold EQUAL or
// NEIGHBOURING byte values in DIFFERENT channels.  In this layout those are the same dword (a broadcast) or dwords next to each
// other (different banks); two lanes collide only when their entries lie a multiple of 128 bytes apart (21.3 byte values), which is
// chance.  Channel planes [3][256] would put equal values of different channels exactly 512 bytes apart -- the same bank, a 3-way
// conflict on every grey pixel -- and an 8-byte entry per value makes the table 2 KB to read 2 bytes of each.  So: the interleaved form.
//
// The bytes.  A batch may start at any byte and a row is 3 w bytes, so almost no run of 8 starts on a dword.  When the 8 values lie
// in one patch row they are 8 contiguous bytes at `a`: the two (a on a dword) or three aligned dwords that cover them are loaded and
// funnel-shifted together (v_alignbyte), as the uint8 stem does.  Each of those dwords holds at least one of the 8 bytes -- for
// a & 3 != 0 the third one holds byte a + 7 -- so it lies in a page of the batch and only its bytes of the batch are used.  A vector
// that crosses into the next patch row (3 p % 8 != 0: patch 14) or into the padding goes byte by byte.
__global__ __launch_bounds__(ET) void vit_patchify_norm_u8_h_kernel(const unsigned char* __restrict__ x, const v4u* __restrict__ table, int h,
                                                                     int w, int p, int kv, long vectors, v4u* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned short lut[256 * 3];
    if (threadIdx.x < 256 * 3 * 2 / 16) reinterpret_cast<v4u*>(lut)[threadIdx.x] = table[threadIdx.x];
    __syncthreads();
    const int run = 3 * p, k_real = run * p, gw = w / p, gh = h / p;
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const int v = (int)(i % kv);
        long t = i / kv;
        const int gx = (int)(t % gw);
        t /= gw;
        const int gy = (int)(t % gh);
        const long b = t / gh;
        int k = 8 * v, ky = k / run, rem = k - ky * run;
        const long base = ((b * h + (long)gy * p) * w + (long)gx * p) * 3;  // the patch's first byte; a row further down is + 3 w
        unsigned short hv[8];
        if (rem + 8 <= run && k + 8 <= k_real) {
            const unsigned char* a = x + base + (long)ky * w * 3 + rem;
            const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(a) & 3u);
            const unsigned* q = reinterpret_cast<const unsigned*>(a - sh);
            unsigned lo = q[0], hi = q[1];
            if (sh != 0) {
                const unsigned top = q[2];
                lo = __builtin_amdgcn_alignbyte(hi, lo, sh);
                hi = __builtin_amdgcn_alignbyte(top, hi, sh);
            }
            int c = rem % 3;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                hv[e] = lut[3 * (((e < 4 ? lo : hi) >> (8 * (e & 3))) & 255u) + c];
                c = c == 2 ? 0 : c + 1;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e, ++k) {
                if (k < k_real) {
                    hv[e] = lut[3 * x[base + (long)ky * w * 3 + rem] + rem % 3];
                    if (++rem == run) rem = 0, ++ky;
                } else {
                    hv[e] = 0;
                }
            }
        }
        v4u o;
        o.x = (unsigned)hv[0] | ((unsigned)hv[1] << 16);
        o.y = (unsigned)hv[2] | ((unsigned)hv[3] << 16);
        o.z = (unsigned)hv[4] | ((unsigned)hv[5] << 16);
        o.w = (unsigned)hv[6] | ((unsigned)hv[7] << 16);
        out[i] = o;
    }
}

// One wave per row, four rows per workgroup, no LDS.  Four classes at a time: lane l multiplies the 16-byte vectors l, l + 64, ... of
// the row (read once per four classes; the row and W stay in cache) into one float32 accumulator per class, in that order, and the
// 64 partial sums are folded by the same exchanges every time -- the order of a logit's additions depends on f alone, not on the
// row, the batch or the grid.  Lane j then keeps logit j (c <= 64), and the softmax is two more folds over the wave: the maximum,
// expf of the difference (lanes from c on contribute 0), the sum, ONE division per element.  c == 1: expf(0) / 1 = 1 exactly.
__global__ __launch_bounds__(ET) void linear_softmax_rows_f32_kernel(const float* __restrict__ x, long stride, const float* __restrict__ wgt,
                                                                      const float* __restrict__ bias, long rows, int f, int c,
                                                                      float* __restrict__ prob) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;  // whole waves leave: the exchanges below stay inside a wave
    const float4* xr = reinterpret_cast<const float4*>(x + row * stride);
    const int fv = f >> 2;
    float logit = -INFINITY;
    for (int j0 = 0; j0 < c; j0 += 4) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int v = lane; v < fv; v += 64) {
            const float4 xv = xr[v];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (j0 + q < c) {
                    const float4 wv = reinterpret_cast<const float4*>(wgt + (long)(j0 + q) * f)[v];
                    acc[q] = fmaf(xv.x, wv.x, acc[q]);
                    acc[q] = fmaf(xv.y, wv.y, acc[q]);
                    acc[q] = fmaf(xv.z, wv.z, acc[q]);
                    acc[q] = fmaf(xv.w, wv.w, acc[q]);
                }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (j0 + q < c) {  // (uniform over the wave)
                const float s = wave_sum(acc[q]) + (bias != nullptr ? bias[j0 + q] : 0.0f);
                if (lane == j0 + q) logit = s;
            }
    }
    const float top = wave_max(logit);
    const float e = lane < c ? expf(logit - top) : 0.0f;
    const float sum = wave_sum(e);
    if (lane < c) prob[row * (long)c + lane] = e / sum;
}

unsigned stream_blocks(long items) {
    long blocks = (items + ET - 1) / ET;
    if (blocks > 256L * 64) blocks = 256L * 64;
    return (unsigned)blocks;
}

}  // namespace

extern "C" int tia_vit_patchify_norm_u8_h(const uint8_t* d_x, const void* d_table, void* d_tokens, int64_t n, int64_t h, int64_t w,
                                          int64_t patch, int64_t k_pad, int32_t dtype, void* stream) {
    if (!d_x || !d_table || !d_tokens || n <= 0 || h <= 0 || w <= 0 || patch <= 0 || k_pad <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (h % patch != 0 || w % patch != 0) return TIA_ESIZE;
    if (h > 0x7fffffffL / 3 || w > 0x7fffffffL / 3 || n > 0x7fffffffL || patch > 16384) return TIA_ESIZE;  // (3 p^2 stays an int)
    if ((k_pad & 31) != 0 || k_pad < 3 * patch * patch || k_pad > 0x7fffffe0L) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_table) | reinterpret_cast<uintptr_t>(d_tokens)) & 15) return TIA_EINVAL;
    const long vectors = n * (h / patch) * (w / patch) * (k_pad / 8);
    // (the table's halves are copied as they are: `dtype` names what they are and is checked, the kernel is the same for both)
    hipLaunchKernelGGL(vit_patchify_norm_u8_h_kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, d_x,
                       static_cast<const v4u*>(d_table), (int)h, (int)w, (int)patch, (int)(k_pad / 8), vectors, static_cast<v4u*>(d_tokens));
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_linear_softmax_rows_f32(const float* d_x, int64_t row_stride, const float* d_w, const float* d_bias, float* d_p,
                                           int64_t rows, int64_t f, int64_t c, void* stream) {
    if (!d_x || !d_w || !d_p || rows <= 0 || f <= 0 || c <= 0) return TIA_EINVAL;
    if (c > 64 || (f & 3) != 0 || f > 8192) return TIA_ESIZE;
    if (row_stride < f || (row_stride & 3) != 0) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_w)) & 15) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_bias) | reinterpret_cast<uintptr_t>(d_p)) & 3) return TIA_EINVAL;
    const long blocks = (rows + ET / 64 - 1) / (ET / 64);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    hipLaunchKernelGGL(linear_softmax_rows_f32_kernel, dim3((unsigned)blocks), dim3(ET), 0, (hipStream_t)stream, d_x, (long)row_stride, d_w,
                       d_bias, (long)rows, (int)f, (int)c, d_p);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
