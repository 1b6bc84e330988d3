// The memory-bound passes of the Vision Transformer graph (fp16 / bf16 activations; models/architecture/vit_fused.py):
//   layernorm_rows  : y[r, :] = (x[r, :] - mean) / sqrt(var + eps) * gamma + beta     rows at a stride, half or float32 out
//   gelu_rows       : x = 0.5 x (1 + erf(x / sqrt 2)) in place
//   vit_patchify    : NHWC image batch -> [n, g, p * p * 3] tokens, k order (ky, kx, c)   float32 or half in, half out
//   assemble_tokens : out[b, 0] = cls + pos[0], out[b, 1 + i] = tok[b, i] + pos[1 + i]
// and what the foundation models (UNI2, H-optimus, prov-gigapath) add to the graph:
//   swiglu_rows      : y[r, j] = silu(x[r, j]) * x[r, H + j]     the packed fc1 output [rows, 2 H] -> [rows, H]
//   vit_patchify_pad : the same im2col for any patch size, rows zero-padded to k_pad columns (a 14-pixel patch: 588 -> 608)
//   assemble_prefix  : out[b] = cat(cls (+ pos[0]), reg[0 .. R), tok[b] + pos[has_cls ..])
// and the output of Virchow / Virchow2:
//   cls_mean_pool    : out[b] = cat(LN(x[b, 0]), mean_{i >= skip} LN(x[b, i]))     float32 out, one workgroup per image
// 16 bytes per lane and access (8 halves), float32 arithmetic, ONE round-to-nearest-even on the way out, 64-bit element offsets.
#include "conv_device.hpp"
#include "half_rows.hpp"
#include "wide_io.hpp"

namespace {

using namespace tia;

constexpr int ET = 256;

// One wave per row, the row in registers (VPL 16-byte vectors per lane, c <= 512 VPL): one read of x, the mean, then the variance
// of the CENTRED values (not E[x^2] - mean^2, which cancels for rows with a large mean), both folded over the wave by lane
// exchanges -- no LDS, no barrier.  Four rows per workgroup.
template <bool BF, bool OUT_F32, int VPL>
__global__ __launch_bounds__(ET) void layernorm_rows_h_kernel(const unsigned short* __restrict__ x, long stride, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, long rows, int c,
                                                               void* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;  // whole waves leave: the exchanges below stay inside a wave
    const int cv = c >> 3;
    const unsigned short* xr = x + row * stride;
    float f[VPL][8];
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            unpack8<BF>(*reinterpret_cast<const v4u*>(xr + 8 * v), f[i]);
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += f[i][k];
        }
    }
    const float mean = wave_sum(sum) / (float)c;
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                f[i][k] -= mean;
                sq = fmaf(f[i][k], f[i][k], sq);
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)c + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            float g[8], bt[8], r[8];
            load8_f32(gamma + 8 * v, g);
            load8_f32(beta + 8 * v, bt);
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] = fmaf(f[i][k] * rstd, g[k], bt[k]);
            if constexpr (OUT_F32) {
                float* yr = static_cast<float*>(y) + row * (long)c + 8 * v;
                *reinterpret_cast<float4*>(yr) = make_float4(r[0], r[1], r[2], r[3]);
                *reinterpret_cast<float4*>(yr + 4) = make_float4(r[4], r[5], r[6], r[7]);
            } else {
                *reinterpret_cast<v4u*>(static_cast<unsigned short*>(y) + row * (long)c + 8 * v) = pack8<BF>(r);
            }
        }
    }
}

template <bool BF>
__global__ __launch_bounds__(ET) void gelu_rows_h_kernel(v4u* __restrict__ x, long vectors) {
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        float f[8];
        unpack8<BF>(x[i], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = 0.5f * f[k] * (1.0f + erff(f[k] * 0.70710678118654752440f));
        x[i] = pack8<BF>(f);
    }
}

// One thread per 8 output halves.  A token's p * p * 3 values are p runs (one per patch row ky) of 3 p contiguous input values, and
// 3 p % 8 == 0, so an output vector is 8 contiguous input values: one 16-byte (half) or two 16-byte (float32) loads.
template <bool BF, bool IN_F32>
__global__ __launch_bounds__(ET) void vit_patchify_h_kernel(const void* __restrict__ x, int h, int w, int p, long vectors, v4u* __restrict__ out) {
    const int run_v = 3 * p / 8, gw = w / p, gh = h / p;
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const int v = (int)(i % run_v);
        long t = i / run_v;
        const int ky = (int)(t % p);
        t /= p;
        const int gx = (int)(t % gw);
        t /= gw;
        const int gy = (int)(t % gh);
        const long b = t / gh;
        const long src = ((b * h + (long)gy * p + ky) * w + (long)gx * p) * 3 + 8 * v;
        if constexpr (IN_F32) {
            float f[8];
            load8_f32(static_cast<const float*>(x) + src, f);
            out[i] = pack8<BF>(f);
        } else {
            out[i] = *reinterpret_cast<const v4u*>(static_cast<const unsigned short*>(x) + src);
        }
    }
}

template <bool BF>
__global__ __launch_bounds__(ET) void vit_assemble_tokens_h_kernel(const v4u* __restrict__ tok, const float* __restrict__ cls,
                                                                    const float* __restrict__ pos, long vectors, int g, int dv,
                                                                    v4u* __restrict__ out) {
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const int v = (int)(i % dv);
        const long t = i / dv;
        const int tk = (int)(t % (g + 1));
        const long b = t / (g + 1);
        float a[8], ps[8];
        if (tk == 0) load8_f32(cls + 8 * v, a);
        else unpack8<BF>(tok[(b * g + (tk - 1)) * dv + v], a);
        load8_f32(pos + ((long)tk * dv + v) * 8, ps);
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] += ps[k];
        out[i] = pack8<BF>(a);
    }
}

// One thread per 8 outputs: the gate vector at [r, 8 j] and the value vector at [r, H + 8 j], both 16-byte loads (H % 8 == 0 makes
// every row and its second half start on a vector), one 16-byte store.
template <bool BF>
__global__ __launch_bounds__(ET) void swiglu_rows_h_kernel(const v4u* __restrict__ x, long vectors, int hv, v4u* __restrict__ y) {
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const long r = i / hv;
        const int j = (int)(i - r * hv);
        float gate[8], val[8];
        unpack8<BF>(x[r * (2L * hv) + j], gate);
        unpack8<BF>(x[r * (2L * hv) + hv + j], val);
#pragma unroll
        for (int k = 0; k < 8; ++k) gate[k] = silu_f32(gate[k]) * val[k];
        y[i] = pack8<BF>(gate);
    }
}

// One thread per 8 output halves of a k_pad-wide token row.  A patch row (3 p values) is no whole number of 16-byte vectors when
// p % 8 != 0 and starts on no 16-byte boundary in the image, so the 8 values are read one by one (4-byte or 2-byte loads, always
// aligned; neighbouring lanes read neighbouring addresses) while (ky, position in the run) steps along; columns from 3 p^2 on are
// written as zeros.  The store is one aligned 16-byte vector (k_pad % 8 == 0).
template <bool BF, bool IN_F32>
__global__ __launch_bounds__(ET) void vit_patchify_pad_h_kernel(const void* __restrict__ x, int h, int w, int p, int kv, long vectors,
                                                                 v4u* __restrict__ out) {
    const int run = 3 * p, k_real = run * p, gw = w / p, gh = h / p;
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const int v = (int)(i % kv);
        long t = i / kv;
        const int gx = (int)(t % gw);
        t /= gw;
        const int gy = (int)(t % gh);
        const long b = t / gh;
        int k = 8 * v, ky = k / run, rem = k - ky * run;
        const long base = ((b * h + (long)gy * p) * w + (long)gx * p) * 3;  // the patch's first value; a row further down is + 3 w
        float f[8];
        unsigned short hv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e, ++k) {
            if (k < k_real) {
                const long src = base + (long)ky * w * 3 + rem;
                if constexpr (IN_F32) f[e] = static_cast<const float*>(x)[src];
                else hv[e] = static_cast<const unsigned short*>(x)[src];
                if (++rem == run) rem = 0, ++ky;
            } else {
                f[e] = 0.0f;
                hv[e] = 0;
            }
        }
        if constexpr (IN_F32) {
            out[i] = pack8<BF>(f);
        } else {
            v4u o;
            o.x = (unsigned)hv[0] | ((unsigned)hv[1] << 16);
            o.y = (unsigned)hv[2] | ((unsigned)hv[3] << 16);
            o.z = (unsigned)hv[4] | ((unsigned)hv[5] << 16);
            o.w = (unsigned)hv[6] | ((unsigned)hv[7] << 16);
            out[i] = o;
        }
    }
}

// vit_assemble_tokens_h_kernel with R register rows after the class row and a position table with or without a class entry
// (has_cls = 1 / 0).  R = 0 with has_cls = 1 is that kernel's arithmetic exactly.
template <bool BF>
__global__ __launch_bounds__(ET) void vit_assemble_prefix_h_kernel(const v4u* __restrict__ tok, const float* __restrict__ cls,
                                                                    const float* __restrict__ reg, const float* __restrict__ pos,
                                                                    int has_cls, long vectors, int g, int nreg, int dv,
                                                                    v4u* __restrict__ out) {
    const int s = 1 + nreg + g;
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const int v = (int)(i % dv);
        const long t = i / dv;
        const int tk = (int)(t % s);
        const long b = t / s;
        float a[8];
        long prow = -1;  // the row of `pos` to add, if any
        if (tk == 0) {
            load8_f32(cls + 8 * v, a);
            if (has_cls) prow = 0;
        } else if (tk <= nreg) {
            load8_f32(reg + ((long)(tk - 1) * dv + v) * 8, a);
        } else {
            const int pi = tk - 1 - nreg;
            unpack8<BF>(tok[(b * g + pi) * dv + v], a);
            prow = pi + has_cls;
        }
        if (prow >= 0) {
            float ps[8];
            load8_f32(pos + (prow * dv + v) * 8, ps);
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] += ps[k];
        }
        out[i] = pack8<BF>(a);
    }
}

// Row `xr` normalised as in layernorm_rows_h_kernel (one read, the mean, then the variance of the centred values, both folded over
// the wave), WITHOUT the affine: f = (x - mean) * rstd in float32, this lane's vectors lane + 64 i.
template <bool BF, int VPL>
__device__ __forceinline__ void normalise_row(const unsigned short* xr, int lane, int cv, int c, float eps, float (&f)[VPL][8]) {
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            unpack8<BF>(*reinterpret_cast<const v4u*>(xr + 8 * v), f[i]);
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += f[i][k];
        }
    }
    const float mean = wave_sum(sum) / (float)c;
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                f[i][k] -= mean;
                sq = fmaf(f[i][k], f[i][k], sq);
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)c + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int k = 0; k < 8; ++k) f[i][k] *= rstd;
        }
}

// Class + mean-patch pooling of the final norm (Virchow / Virchow2): out[b, :d] = LN(x[b, 0]), out[b, d:] = mean_{i >= skip} LN(x[b, i]).
// One workgroup per image.  Wave w normalises rows skip + w, skip + w + 4, ... (a row per wave, in registers, as above) and adds each
// to per-lane float32 accumulators in that order; wave 0 writes the class row first.  The four partial sums are folded through one
// LDS row in wave order, ((w0 + w1) + w2) + w3, and the affine is applied ONCE to the mean: mean_i (g y_i + b) = g mean_i y_i + b, so
// the sum runs over the normalised values alone.  No atomics, nothing depends on the grid: an image's result does not depend on n.
template <bool BF, int VPL>
__global__ __launch_bounds__(ET) void vit_cls_mean_pool_h_kernel(const unsigned short* __restrict__ x, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float eps, int s, int skip, int c,
                                                                  float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float pool_fold[];  // [c]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cv = c >> 3;
    const unsigned short* xb = x + (long)blockIdx.x * s * c;
    float* ob = out + (long)blockIdx.x * 2 * c;
    float f[VPL][8], acc[VPL][8];
#pragma unroll
    for (int i = 0; i < VPL; ++i)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[i][k] = 0.0f;

    if (wave == 0) {  // (a whole wave: the exchanges stay inside it)
        normalise_row<BF, VPL>(xb, lane, cv, c, eps, f);
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int v = lane + 64 * i;
            if (v < cv) {
                float g[8], bt[8];
                load8_f32(gamma + 8 * v, g);
                load8_f32(beta + 8 * v, bt);
                *reinterpret_cast<float4*>(ob + 8 * v) = make_float4(fmaf(f[i][0], g[0], bt[0]), fmaf(f[i][1], g[1], bt[1]),
                                                                     fmaf(f[i][2], g[2], bt[2]), fmaf(f[i][3], g[3], bt[3]));
                *reinterpret_cast<float4*>(ob + 8 * v + 4) = make_float4(fmaf(f[i][4], g[4], bt[4]), fmaf(f[i][5], g[5], bt[5]),
                                                                         fmaf(f[i][6], g[6], bt[6]), fmaf(f[i][7], g[7], bt[7]));
            }
        }
    }
    for (int row = skip + wave; row < s; row += ET / 64) {
        normalise_row<BF, VPL>(xb + (long)row * c, lane, cv, c, eps, f);
#pragma unroll
        for (int i = 0; i < VPL; ++i)
            if (lane + 64 * i < cv) {
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[i][k] += f[i][k];
            }
    }
    // the fold: wave 0 lays its sums down, waves 1, 2 add theirs in turn, wave 3 adds its own and writes the mean
    for (int w = 0; w < ET / 64; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const int v = lane + 64 * i;
                if (v < cv) {
                    if (w > 0) {
                        float p[8];
                        load8_f32(pool_fold + 8 * v, p);
#pragma unroll
                        for (int k = 0; k < 8; ++k) acc[i][k] = p[k] + acc[i][k];
                    }
                    if (w < ET / 64 - 1) {
                        *reinterpret_cast<float4*>(pool_fold + 8 * v) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
                        *reinterpret_cast<float4*>(pool_fold + 8 * v + 4) = make_float4(acc[i][4], acc[i][5], acc[i][6], acc[i][7]);
                    } else {
                        const float cnt = (float)(s - skip);
                        float g[8], bt[8], r[8];
                        load8_f32(gamma + 8 * v, g);
                        load8_f32(beta + 8 * v, bt);
#pragma unroll
                        for (int k = 0; k < 8; ++k) r[k] = fmaf(acc[i][k] / cnt, g[k], bt[k]);
                        *reinterpret_cast<float4*>(ob + c + 8 * v) = make_float4(r[0], r[1], r[2], r[3]);
                        *reinterpret_cast<float4*>(ob + c + 8 * v + 4) = make_float4(r[4], r[5], r[6], r[7]);
                    }
                }
            }
        }
        __syncthreads();
    }
}

unsigned stream_blocks(long items) {
    long blocks = (items + ET - 1) / ET;
    if (blocks > 256L * 64) blocks = 256L * 64;
    return (unsigned)blocks;
}

template <bool BF, bool OUT_F32>
void launch_layernorm(int vpl, dim3 grid, hipStream_t st, const unsigned short* x, long stride, const float* gamma, const float* beta, float eps,
                      long rows, int c, void* y) {
#define TIA_LN(V) hipLaunchKernelGGL((layernorm_rows_h_kernel<BF, OUT_F32, V>), grid, dim3(ET), 0, st, x, stride, gamma, beta, eps, rows, c, y)
    if (vpl <= 1) TIA_LN(1);
    else if (vpl <= 2) TIA_LN(2);
    else if (vpl <= 4) TIA_LN(4);
    else if (vpl <= 8) TIA_LN(8);
    else TIA_LN(16);
#undef TIA_LN
}

}  // namespace

extern "C" int tia_layernorm_rows_h(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, void* d_y,
                                    int64_t rows, int64_t c, int32_t dtype, int32_t out_f32, void* stream) {
    if (!d_x || !d_gamma || !d_beta || !d_y || rows <= 0 || c <= 0 || !(eps >= 0.0f)) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((c & 7) != 0 || c > 8192) return TIA_ESIZE;
    if (row_stride < c || (row_stride & 7) != 0) return TIA_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_gamma) | reinterpret_cast<uintptr_t>(d_beta) |
         reinterpret_cast<uintptr_t>(d_y)) & 15)
        return TIA_EINVAL;
    const long blocks = (rows + ET / 64 - 1) / (ET / 64);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    const int vpl = (int)((c / 8 + 63) / 64);
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    const unsigned short* x = static_cast<const unsigned short*>(d_x);
    const bool bf = dtype == TIA_DT_BF16;
    if (out_f32) {
        if (bf) launch_layernorm<true, true>(vpl, grid, st, x, (long)row_stride, d_gamma, d_beta, eps, (long)rows, (int)c, d_y);
        else launch_layernorm<false, true>(vpl, grid, st, x, (long)row_stride, d_gamma, d_beta, eps, (long)rows, (int)c, d_y);
    } else {
        if (bf) launch_layernorm<true, false>(vpl, grid, st, x, (long)row_stride, d_gamma, d_beta, eps, (long)rows, (int)c, d_y);
        else launch_layernorm<false, false>(vpl, grid, st, x, (long)row_stride, d_gamma, d_beta, eps, (long)rows, (int)c, d_y);
    }
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_cls_mean_pool_h(const void* d_x, const float* d_gamma, const float* d_beta, float eps, float* d_out, int64_t n,
                                       int64_t s, int64_t skip, int64_t d, int32_t dtype, void* stream) {
    if (!d_x || !d_gamma || !d_beta || !d_out || n <= 0 || s <= 0 || d <= 0 || !(eps >= 0.0f)) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (skip < 1 || skip >= s) return TIA_EINVAL;
    if ((d & 7) != 0 || d > 8192) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_gamma) | reinterpret_cast<uintptr_t>(d_beta) |
         reinterpret_cast<uintptr_t>(d_out)) & 15)
        return TIA_EINVAL;
    if (n > 0x7fffffffL || s > 0x7fffffffL) return TIA_ESIZE;  // one grid dimension; the row index is an int
    const int vpl = (int)((d / 8 + 63) / 64);
    const dim3 grid((unsigned)n);
    const size_t lds = (size_t)d * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    const unsigned short* x = static_cast<const unsigned short*>(d_x);
#define TIA_POOL(BF, V) \
    hipLaunchKernelGGL((vit_cls_mean_pool_h_kernel<BF, V>), grid, dim3(ET), lds, st, x, d_gamma, d_beta, eps, (int)s, (int)skip, (int)d, d_out)
#define TIA_POOL_V(BF)            \
    do {                          \
        if (vpl <= 1) TIA_POOL(BF, 1);       \
        else if (vpl <= 2) TIA_POOL(BF, 2);  \
        else if (vpl <= 4) TIA_POOL(BF, 4);  \
        else if (vpl <= 8) TIA_POOL(BF, 8);  \
        else TIA_POOL(BF, 16);               \
    } while (0)
    if (dtype == TIA_DT_BF16) TIA_POOL_V(true);
    else TIA_POOL_V(false);
#undef TIA_POOL_V
#undef TIA_POOL
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_gelu_rows_h(void* d_x, int64_t count, int32_t dtype, void* stream) {
    if (!d_x || count <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((count & 7) != 0) return TIA_ESIZE;
    if (reinterpret_cast<uintptr_t>(d_x) & 15) return TIA_EINVAL;
    const long vectors = count / 8;
    const auto kernel = dtype == TIA_DT_BF16 ? gelu_rows_h_kernel<true> : gelu_rows_h_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, (v4u*)d_x, vectors);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_patchify_h(const void* d_x, int32_t x_dtype, void* d_tokens, int64_t n, int64_t h, int64_t w, int64_t patch,
                                  int32_t dtype, void* stream) {
    if (!d_x || !d_tokens || n <= 0 || h <= 0 || w <= 0 || patch <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (x_dtype != TIA_DT_F32 && x_dtype != dtype) return TIA_EINVAL;
    if ((patch & 7) != 0 || h % patch != 0 || w % patch != 0) return TIA_ESIZE;  // 3 p values of a patch row = whole 16-byte vectors
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_tokens)) & 15) return TIA_EINVAL;
    if (h > 0x7fffffffL / 3 || w > 0x7fffffffL / 3 || n > 0x7fffffffL) return TIA_ESIZE;
    const long vectors = n * h * w * 3 / 8;
    const unsigned blocks = stream_blocks(vectors);
    hipStream_t st = (hipStream_t)stream;
    const bool bf = dtype == TIA_DT_BF16, in32 = x_dtype == TIA_DT_F32;
    using Kernel = void (*)(const void*, int, int, int, long, v4u*);
    const Kernel kernels[2][2] = {{vit_patchify_h_kernel<false, false>, vit_patchify_h_kernel<false, true>},
                                  {vit_patchify_h_kernel<true, false>, vit_patchify_h_kernel<true, true>}};
    hipLaunchKernelGGL(kernels[bf][in32], dim3(blocks), dim3(ET), 0, st, d_x, (int)h, (int)w, (int)patch, vectors, (v4u*)d_tokens);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_assemble_tokens_h(const void* d_tokens, const float* d_cls, const float* d_pos, void* d_out, int64_t n, int64_t g,
                                         int64_t d, int32_t dtype, void* stream) {
    if (!d_tokens || !d_cls || !d_pos || !d_out || n <= 0 || g <= 0 || d <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((d & 7) != 0) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_tokens) | reinterpret_cast<uintptr_t>(d_cls) | reinterpret_cast<uintptr_t>(d_pos) |
         reinterpret_cast<uintptr_t>(d_out)) & 15)
        return TIA_EINVAL;
    if (g > 0x7ffffffeL || d > 0x7fffffffL || n > 0x7fffffffL) return TIA_ESIZE;
    const long vectors = n * (g + 1) * (d / 8);
    const auto kernel = dtype == TIA_DT_BF16 ? vit_assemble_tokens_h_kernel<true> : vit_assemble_tokens_h_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, (const v4u*)d_tokens, d_cls, d_pos, vectors,
                       (int)g, (int)(d / 8), (v4u*)d_out);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_swiglu_rows_h(const void* d_x, void* d_y, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    if (!d_x || !d_y || rows <= 0 || hidden <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((hidden & 7) != 0 || hidden > 0x3fffffffL || rows > 0x7fffffffL) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y)) & 15) return TIA_EINVAL;
    const long vectors = rows * (hidden / 8);
    const auto kernel = dtype == TIA_DT_BF16 ? swiglu_rows_h_kernel<true> : swiglu_rows_h_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, (const v4u*)d_x, vectors, (int)(hidden / 8),
                       (v4u*)d_y);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_patchify_pad_h(const void* d_x, int32_t x_dtype, void* d_tokens, int64_t n, int64_t h, int64_t w, int64_t patch,
                                      int64_t k_pad, int32_t dtype, void* stream) {
    if (!d_x || !d_tokens || n <= 0 || h <= 0 || w <= 0 || patch <= 0 || k_pad <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (x_dtype != TIA_DT_F32 && x_dtype != dtype) return TIA_EINVAL;
    if (h % patch != 0 || w % patch != 0) return TIA_ESIZE;
    if (h > 0x7fffffffL / 3 || w > 0x7fffffffL / 3 || n > 0x7fffffffL || patch > 16384) return TIA_ESIZE;  // (3 p^2 stays an int)
    if ((k_pad & 31) != 0 || k_pad < 3 * patch * patch || k_pad > 0x7fffffe0L) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_tokens)) & 15) return TIA_EINVAL;
    const long vectors = n * (h / patch) * (w / patch) * (k_pad / 8);
    hipStream_t st = (hipStream_t)stream;
    const bool bf = dtype == TIA_DT_BF16, in32 = x_dtype == TIA_DT_F32;
    using Kernel = void (*)(const void*, int, int, int, int, long, v4u*);
    const Kernel kernels[2][2] = {{vit_patchify_pad_h_kernel<false, false>, vit_patchify_pad_h_kernel<false, true>},
                                  {vit_patchify_pad_h_kernel<true, false>, vit_patchify_pad_h_kernel<true, true>}};
    hipLaunchKernelGGL(kernels[bf][in32], dim3(stream_blocks(vectors)), dim3(ET), 0, st, d_x, (int)h, (int)w, (int)patch, (int)(k_pad / 8),
                       vectors, (v4u*)d_tokens);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_assemble_prefix_h(const void* d_tokens, const float* d_cls, const float* d_reg, const float* d_pos,
                                         int32_t pos_has_cls, void* d_out, int64_t n, int64_t g, int64_t reg_tokens, int64_t d,
                                         int32_t dtype, void* stream) {
    if (!d_tokens || !d_cls || !d_pos || !d_out || n <= 0 || g <= 0 || d <= 0 || reg_tokens < 0) return TIA_EINVAL;
    if ((reg_tokens > 0) != (d_reg != nullptr) || (pos_has_cls != 0 && pos_has_cls != 1)) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((d & 7) != 0) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_tokens) | reinterpret_cast<uintptr_t>(d_cls) | reinterpret_cast<uintptr_t>(d_reg) |
         reinterpret_cast<uintptr_t>(d_pos) | reinterpret_cast<uintptr_t>(d_out)) & 15)
        return TIA_EINVAL;
    if (g > 0x3fffffffL || reg_tokens > 0x3fffffffL || d > 0x7fffffffL || n > 0x7fffffffL) return TIA_ESIZE;
    const long vectors = n * (1 + reg_tokens + g) * (d / 8);
    const auto kernel = dtype == TIA_DT_BF16 ? vit_assemble_prefix_h_kernel<true> : vit_assemble_prefix_h_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, (const v4u*)d_tokens, d_cls, d_reg, d_pos,
                       (int)pos_has_cls, vectors, (int)g, (int)reg_tokens, (int)(d / 8), (v4u*)d_out);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// residual_dtype="float32": the residual stream x is a float32 [n, S, D] tensor and the GEMMs write half BRANCHES (no residual in
// their epilogues).  Three kernels, each the float32-stream form of one above; the kernels above are untouched.
//   add_layernorm_rows_f32 : x += float(branch) in place (one float32 add, never rounded), y = LN(x)     either part optional
//   vit_assemble_rows_f32  : assemble_prefix with a float32 result: float(tok) + pos, not rounded
//   cls_mean_pool_f32      : cls_mean_pool of x (+ float(branch) on load, not written back)
// ------------------------------------------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ void store8_f32(float* p, const float (&r)[8]) {
    *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(r[4], r[5], r[6], r[7]);
}

// layernorm_rows_h_kernel on a float32 row (two 16-byte loads per vector of 8), with the branch added first: the lane that reads
// x[8 v .. 8 v + 8) adds the branch's 8 halves and writes the same 8 floats back, so the update is in place without any exchange.
// YMODE 0: no LayerNorm (the add alone), 1: y in the half type BF (one rounding), 2: y in float32.  `branch` may be null (LayerNorm
// alone: x is only read).  The mean, the centred variance and the affine are that kernel's, operation for operation.
template <bool BF, int YMODE, int VPL>
__global__ __launch_bounds__(ET) void add_layernorm_rows_f32_kernel(float* __restrict__ x, long xstride, const unsigned short* __restrict__ branch,
                                                                     long bstride, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float eps, long rows, int c,
                                                                     void* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;  // whole waves leave: the exchanges below stay inside a wave
    const int cv = c >> 3;
    float* xr = x + row * xstride;
    const unsigned short* br = branch ? branch + row * bstride : nullptr;
    float f[VPL][8];
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            load8_f32(xr + 8 * v, f[i]);
            if (br) {
                float b[8];
                unpack8<BF>(*reinterpret_cast<const v4u*>(br + 8 * v), b);
#pragma unroll
                for (int k = 0; k < 8; ++k) f[i][k] += b[k];
                store8_f32(xr + 8 * v, f[i]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += f[i][k];
        }
    }
    if constexpr (YMODE != 0) {
        const float mean = wave_sum(sum) / (float)c;
        float sq = 0.0f;
#pragma unroll
        for (int i = 0; i < VPL; ++i)
            if (lane + 64 * i < cv) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    f[i][k] -= mean;
                    sq = fmaf(f[i][k], f[i][k], sq);
                }
            }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)c + eps);
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int v = lane + 64 * i;
            if (v < cv) {
                float g[8], bt[8], r[8];
                load8_f32(gamma + 8 * v, g);
                load8_f32(beta + 8 * v, bt);
#pragma unroll
                for (int k = 0; k < 8; ++k) r[k] = fmaf(f[i][k] * rstd, g[k], bt[k]);
                if constexpr (YMODE == 2) store8_f32(static_cast<float*>(y) + row * (long)c + 8 * v, r);
                else *reinterpret_cast<v4u*>(static_cast<unsigned short*>(y) + row * (long)c + 8 * v) = pack8<BF>(r);
            }
        }
    }
}

// vit_assemble_prefix_h_kernel with a float32 result: the same rows, the same single float32 add, no rounding after it.
template <bool BF>
__global__ __launch_bounds__(ET) void vit_assemble_rows_f32_kernel(const v4u* __restrict__ tok, const float* __restrict__ cls,
                                                                    const float* __restrict__ reg, const float* __restrict__ pos,
                                                                    int has_cls, long vectors, int g, int nreg, int dv,
                                                                    float* __restrict__ out) {
    const int s = 1 + nreg + g;
    for (long i = (long)blockIdx.x * ET + threadIdx.x; i < vectors; i += (long)gridDim.x * ET) {
        const int v = (int)(i % dv);
        const long t = i / dv;
        const int tk = (int)(t % s);
        const long b = t / s;
        float a[8];
        long prow = -1;  // the row of `pos` to add, if any
        if (tk == 0) {
            load8_f32(cls + 8 * v, a);
            if (has_cls) prow = 0;
        } else if (tk <= nreg) {
            load8_f32(reg + ((long)(tk - 1) * dv + v) * 8, a);
        } else {
            const int pi = tk - 1 - nreg;
            unpack8<BF>(tok[(b * g + pi) * dv + v], a);
            prow = pi + has_cls;
        }
        if (prow >= 0) {
            float ps[8];
            load8_f32(pos + (prow * dv + v) * 8, ps);
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] += ps[k];
        }
        store8_f32(out + i * 8, a);
    }
}

// normalise_row on a float32 row with an optional half branch row added on load (one float32 add per element, nothing written).
template <bool BF, int VPL>
__device__ __forceinline__ void normalise_row_f32(const float* xr, const unsigned short* br, int lane, int cv, int c, float eps,
                                                  float (&f)[VPL][8]) {
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            load8_f32(xr + 8 * v, f[i]);
            if (br) {
                float b[8];
                unpack8<BF>(*reinterpret_cast<const v4u*>(br + 8 * v), b);
#pragma unroll
                for (int k = 0; k < 8; ++k) f[i][k] += b[k];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += f[i][k];
        }
    }
    const float mean = wave_sum(sum) / (float)c;
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                f[i][k] -= mean;
                sq = fmaf(f[i][k], f[i][k], sq);
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)c + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int k = 0; k < 8; ++k) f[i][k] *= rstd;
        }
}

// vit_cls_mean_pool_h_kernel on the float32 stream: the same wave-to-row assignment, the same ((w0 + w1) + w2) + w3 fold through one
// LDS row, the affine applied once to the mean.  `branch` (the last block's fc2 output, [n, s, c] halves) may be null.
template <bool BF, int VPL>
__global__ __launch_bounds__(ET) void vit_cls_mean_pool_f32_kernel(const float* __restrict__ x, const unsigned short* __restrict__ branch,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                    float eps, int s, int skip, int c, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float pool_fold32[];  // [c]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cv = c >> 3;
    const float* xb = x + (long)blockIdx.x * s * c;
    const unsigned short* bb = branch ? branch + (long)blockIdx.x * s * c : nullptr;
    float* ob = out + (long)blockIdx.x * 2 * c;
    float f[VPL][8], acc[VPL][8];
#pragma unroll
    for (int i = 0; i < VPL; ++i)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[i][k] = 0.0f;

    if (wave == 0) {  // (a whole wave: the exchanges stay inside it)
        normalise_row_f32<BF, VPL>(xb, bb, lane, cv, c, eps, f);
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
            const int v = lane + 64 * i;
            if (v < cv) {
                float g[8], bt[8], r[8];
                load8_f32(gamma + 8 * v, g);
                load8_f32(beta + 8 * v, bt);
#pragma unroll
                for (int k = 0; k < 8; ++k) r[k] = fmaf(f[i][k], g[k], bt[k]);
                store8_f32(ob + 8 * v, r);
            }
        }
    }
    for (int row = skip + wave; row < s; row += ET / 64) {
        normalise_row_f32<BF, VPL>(xb + (long)row * c, bb ? bb + (long)row * c : nullptr, lane, cv, c, eps, f);
#pragma unroll
        for (int i = 0; i < VPL; ++i)
            if (lane + 64 * i < cv) {
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[i][k] += f[i][k];
            }
    }
    // the fold: wave 0 lays its sums down, waves 1, 2 add theirs in turn, wave 3 adds its own and writes the mean
    for (int w = 0; w < ET / 64; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < VPL; ++i) {
                const int v = lane + 64 * i;
                if (v < cv) {
                    if (w > 0) {
                        float p[8];
                        load8_f32(pool_fold32 + 8 * v, p);
#pragma unroll
                        for (int k = 0; k < 8; ++k) acc[i][k] = p[k] + acc[i][k];
                    }
                    if (w < ET / 64 - 1) {
                        store8_f32(pool_fold32 + 8 * v, acc[i]);
                    } else {
                        const float cnt = (float)(s - skip);
                        float g[8], bt[8], r[8];
                        load8_f32(gamma + 8 * v, g);
                        load8_f32(beta + 8 * v, bt);
#pragma unroll
                        for (int k = 0; k < 8; ++k) r[k] = fmaf(acc[i][k] / cnt, g[k], bt[k]);
                        store8_f32(ob + c + 8 * v, r);
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <bool BF, int YMODE>
void launch_add_layernorm(int vpl, dim3 grid, hipStream_t st, float* x, long xstride, const unsigned short* branch, long bstride,
                          const float* gamma, const float* beta, float eps, long rows, int c, void* y) {
#define TIA_ALN(V) \
    hipLaunchKernelGGL((add_layernorm_rows_f32_kernel<BF, YMODE, V>), grid, dim3(ET), 0, st, x, xstride, branch, bstride, gamma, beta, eps, rows, c, y)
    if (vpl <= 1) TIA_ALN(1);
    else if (vpl <= 2) TIA_ALN(2);
    else if (vpl <= 4) TIA_ALN(4);
    else if (vpl <= 8) TIA_ALN(8);
    else TIA_ALN(16);
#undef TIA_ALN
}

}  // namespace

extern "C" int tia_add_layernorm_rows_f32(float* d_x, int64_t x_row_stride, const void* d_branch, int64_t branch_row_stride,
                                          const float* d_gamma, const float* d_beta, float eps, void* d_y, int32_t y_dtype, int64_t rows,
                                          int64_t c, int32_t dtype, void* stream) {
    if (!d_x || rows <= 0 || c <= 0 || (!d_branch && !d_y)) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (d_y && (!d_gamma || !d_beta || !(eps >= 0.0f) || (y_dtype != dtype && y_dtype != TIA_DT_F32))) return TIA_EINVAL;
    if ((c & 7) != 0 || c > 8192) return TIA_ESIZE;
    if (x_row_stride < c || (x_row_stride & 3) != 0) return TIA_EINVAL;
    if (d_branch && (branch_row_stride < c || (branch_row_stride & 7) != 0)) return TIA_EINVAL;
    uintptr_t bits = reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_branch);
    if (d_y) bits |= reinterpret_cast<uintptr_t>(d_gamma) | reinterpret_cast<uintptr_t>(d_beta) | reinterpret_cast<uintptr_t>(d_y);
    if (bits & 15) return TIA_EINVAL;
    const long blocks = (rows + ET / 64 - 1) / (ET / 64);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    const int vpl = (int)((c / 8 + 63) / 64);
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    const unsigned short* branch = static_cast<const unsigned short*>(d_branch);
    const bool bf = dtype == TIA_DT_BF16;
#define TIA_ALN_Y(YMODE)                                                                                                                  \
    do {                                                                                                                                  \
        if (bf) launch_add_layernorm<true, YMODE>(vpl, grid, st, d_x, (long)x_row_stride, branch, (long)branch_row_stride, d_gamma, d_beta, \
                                                  eps, (long)rows, (int)c, d_y);                                                          \
        else launch_add_layernorm<false, YMODE>(vpl, grid, st, d_x, (long)x_row_stride, branch, (long)branch_row_stride, d_gamma, d_beta,  \
                                                eps, (long)rows, (int)c, d_y);                                                            \
    } while (0)
    if (!d_y) TIA_ALN_Y(0);
    else if (y_dtype == TIA_DT_F32) TIA_ALN_Y(2);
    else TIA_ALN_Y(1);
#undef TIA_ALN_Y
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_assemble_rows_f32(const void* d_tokens, const float* d_cls, const float* d_reg, const float* d_pos,
                                         int32_t pos_has_cls, float* d_out, int64_t n, int64_t g, int64_t reg_tokens, int64_t d,
                                         int32_t dtype, void* stream) {
    if (!d_tokens || !d_cls || !d_pos || !d_out || n <= 0 || g <= 0 || d <= 0 || reg_tokens < 0) return TIA_EINVAL;
    if ((reg_tokens > 0) != (d_reg != nullptr) || (pos_has_cls != 0 && pos_has_cls != 1)) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((d & 7) != 0 || d > 8192) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_tokens) | reinterpret_cast<uintptr_t>(d_cls) | reinterpret_cast<uintptr_t>(d_reg) |
         reinterpret_cast<uintptr_t>(d_pos) | reinterpret_cast<uintptr_t>(d_out)) & 15)
        return TIA_EINVAL;
    if (g > 0x3fffffffL || reg_tokens > 0x3fffffffL || n > 0x7fffffffL) return TIA_ESIZE;
    const long vectors = n * (1 + reg_tokens + g) * (d / 8);
    const auto kernel = dtype == TIA_DT_BF16 ? vit_assemble_rows_f32_kernel<true> : vit_assemble_rows_f32_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(stream_blocks(vectors)), dim3(ET), 0, (hipStream_t)stream, (const v4u*)d_tokens, d_cls, d_reg, d_pos,
                       (int)pos_has_cls, vectors, (int)g, (int)reg_tokens, (int)(d / 8), d_out);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_vit_cls_mean_pool_f32(const float* d_x, const void* d_branch, const float* d_gamma, const float* d_beta, float eps,
                                         float* d_out, int64_t n, int64_t s, int64_t skip, int64_t d, int32_t dtype, void* stream) {
    if (!d_x || !d_gamma || !d_beta || !d_out || n <= 0 || s <= 0 || d <= 0 || !(eps >= 0.0f)) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if (skip < 1 || skip >= s) return TIA_EINVAL;
    if ((d & 7) != 0 || d > 8192) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_branch) | reinterpret_cast<uintptr_t>(d_gamma) |
         reinterpret_cast<uintptr_t>(d_beta) | reinterpret_cast<uintptr_t>(d_out)) & 15)
        return TIA_EINVAL;
    if (n > 0x7fffffffL || s > 0x7fffffffL) return TIA_ESIZE;  // one grid dimension; the row index is an int
    const int vpl = (int)((d / 8 + 63) / 64);
    const dim3 grid((unsigned)n);
    const size_t lds = (size_t)d * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    const unsigned short* branch = static_cast<const unsigned short*>(d_branch);
#define TIA_POOL32(BF, V) \
    hipLaunchKernelGGL((vit_cls_mean_pool_f32_kernel<BF, V>), grid, dim3(ET), lds, st, d_x, branch, d_gamma, d_beta, eps, (int)s, (int)skip, (int)d, d_out)
#define TIA_POOL32_V(BF)                   \
    do {                                   \
        if (vpl <= 1) TIA_POOL32(BF, 1);       \
        else if (vpl <= 2) TIA_POOL32(BF, 2);  \
        else if (vpl <= 4) TIA_POOL32(BF, 4);  \
        else if (vpl <= 8) TIA_POOL32(BF, 8);  \
        else TIA_POOL32(BF, 16);               \
    } while (0)
    if (dtype == TIA_DT_BF16) TIA_POOL32_V(true);
    else TIA_POOL32_V(false);
#undef TIA_POOL32_V
#undef TIA_POOL32
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}
