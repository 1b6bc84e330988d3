// The Vision Transformer linear layers on the INT8 matrix instruction (models/architecture/vit_fused.py, linear_dtype="int8";
// DESIGN 4.38).  W8A8, symmetric, one scale per token and one per output channel:
//   one row     v[0 .. K) float32:  amax = max |v| (a NaN in the row makes amax NaN);  inv = 127 / amax and s = amax / 127, one
//               float32 division each (amax == 0: inv = s = 1);  q[k] = clamp(rne(v[k] * inv), -127, 127), the product in float32, a
//               NaN product -> code 0; the code -128 is never made.  Stored as q (K bytes of int8) and s (one float32)
//   non-finite  a row holding NaN has s = NaN, a row holding +-inf (and no NaN) s = +inf: every output of that token is non-finite
//   weights     one row per output channel, quantised once from the float32 (LayerScale-folded, SwiGLU-padded) weights
//   activations one row per token, quantised from the float32 value the producing kernel holds, before any rounding to half
//   GEMM        acc[r,o] = sum_k qa[r,k] qw[o,k] exactly in int32 (K <= 65536: K 127^2 < 2^31);
//               y[r,o] = half_rne(float(acc) * sa[r] * sw[o] + bias[o] (+ float32(residual[r,o]))), float(acc) to nearest even
// on v_mfma_i32_16x16x64_i8, two instructions per 128-deep K-step.
//   linear_int8_rows          the GEMM
//   linear_int8_pack_weights  float32 [N, K] -> codes [N, K] + scales [N]
//   layernorm_rows_qi8        LayerNorm of half rows -> codes + scales            (feeds qkv and fc1)
//   gelu_rows_qi8             half fc1 output -> exact GELU in float32 -> codes + scales      (feeds fc2)
//   swiglu_rows_qi8           half packed fc1 output [rows, 2H] -> silu(gate) * value -> codes [rows, H] + scales
// The arithmetic of the three producers up to the float32 value is that of the _h kernels of vit_rows.hip; the GEMM's structure
// (tile, staging, LDS image, epilogue) is linear_fp8_rows_kernel's (vit_fp8.hip), whose few shared helper lines are repeated here so
// that file's instruction streams stay what they were.
#include "conv_device.hpp"
#include "wide_io.hpp"

namespace {

using namespace tia;

using v4i = __attribute__((ext_vector_type(4))) int;
using v2u = __attribute__((ext_vector_type(2))) unsigned;

constexpr int ET = 256;
constexpr float I8_MAX = 127.0f;

// ---- the GEMM -------------------------------------------------------------------------------------------------------------------
// A workgroup of four waves makes a tile of 128 output channels x 128 tokens; a wave a quarter of 64 x 64 as 4 x 4 MFMA tiles.  The
// WEIGHTS are the instruction's A operand and the tokens its B operand: D then has the token on the lane (lane & 15) and four
// CONSECUTIVE channels (4 (lane >> 4) + register) in a lane's four registers, which the epilogue stores as one 8-byte vector.
// Both operands are [row][K] bytes in memory and are staged alike: per 128-deep K-step 128 rows x 128 bytes each, fetched as 16-byte
// pieces into registers one step ahead (in flight during the step's MFMAs) and written to an LDS image of 8 pieces per row with
// the piece index XORed with row & 7.  The instruction takes 16 bytes per lane and operand, so a K-step is two of them: the first on
// piece 2 (lane >> 4) of row lane & 15, the second on piece 2 (lane >> 4) + 1, for BOTH operands: the sum over k pairs byte j of
// A's lane with byte j of B's lane, so the result does not depend on which k the hardware assigns to a byte as long as it does so
// alike for A and B (the exact tests are the check of that).  The int32 sum is exact, whatever the order.
// Rows beyond the operand's end are read from its last row (in range, never stored): a row of a GEMM only reaches its own outputs.
constexpr int BT = 128;                 // tile side, both ways
constexpr int PIECES = BT * 8;          // 16-byte pieces of one operand's K-step
constexpr int64_t K_MAX = 65536;        // K 127^2 stays inside int32

template <bool BF>
__global__ __launch_bounds__(ET) void linear_int8_rows_kernel(const signed char* __restrict__ a, const float* __restrict__ sa,
                                                               const signed char* __restrict__ w, const float* __restrict__ sw,
                                                               const float* __restrict__ bias, const unsigned short* __restrict__ res,
                                                               unsigned short* __restrict__ y, long rows, int n, int k, int n_ct) {
    __shared__ v4u lds[2 * PIECES];  // [0, PIECES): weights, [PIECES, 2 PIECES): tokens
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)(blockIdx.x % n_ct) * BT;
    const long t0 = (long)(blockIdx.x / n_ct) * BT;

    // staging: thread t carries piece t & 7 of rows (t >> 3) + 32 i, i = 0 .. 3, of each operand
    const int srow = tid >> 3, piece = tid & 7;
    const signed char* wsrc[4];
    const signed char* asrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int wr = min(c0 + srow + 32 * i, n - 1);
        const long ar = min(t0 + srow + 32 * i, rows - 1);
        wsrc[i] = w + (long)wr * k + 16 * piece;
        asrc[i] = a + ar * k + 16 * piece;
    }
    const int sdst = srow * 8 + (piece ^ (srow & 7));
    v4u wreg[4], areg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        wreg[i] = *reinterpret_cast<const v4u*>(wsrc[i]);
        areg[i] = *reinterpret_cast<const v4u*>(asrc[i]);
    }

    const int r = lane & 15, g = lane >> 4;
    const int wm = wave & 1, wt = wave >> 1;
    const int p0 = (2 * g) ^ (r & 7), p1 = (2 * g + 1) ^ (r & 7);
    v4i acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) acc[mi][ti] = v4i{0, 0, 0, 0};

    const int steps = k / 128;
    for (int kt = 0; kt < steps; ++kt) {
        __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lds[sdst + 256 * i] = wreg[i];
            lds[PIECES + sdst + 256 * i] = areg[i];
        }
        __syncthreads();
        if (kt + 1 < steps) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                wreg[i] = *reinterpret_cast<const v4u*>(wsrc[i] + 128L * (kt + 1));
                areg[i] = *reinterpret_cast<const v4u*>(asrc[i] + 128L * (kt + 1));
            }
        }
        v4i tlo[4], thi[4];
#pragma unroll
        for (int ti = 0; ti < 4; ++ti) {
            const int row = wt * 64 + ti * 16 + r;
            const v4u lo = lds[PIECES + row * 8 + p0], hi = lds[PIECES + row * 8 + p1];
            tlo[ti] = v4i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w};
            thi[ti] = v4i{(int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = wm * 64 + mi * 16 + r;
            const v4u lo = lds[row * 8 + p0], hi = lds[row * 8 + p1];
            const v4i wlo = v4i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w};
            const v4i whi = v4i{(int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) {
                acc[mi][ti] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wlo, tlo[ti], acc[mi][ti], 0, 0, 0);
                acc[mi][ti] = __builtin_amdgcn_mfma_i32_16x16x64_i8(whi, thi[ti], acc[mi][ti], 0, 0, 0);
            }
        }
    }

    // epilogue: lane = token (r) x four consecutive channels (4 g ..); n % 16 == 0 keeps a lane's four channels on one side of n
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) {
        const long tok = t0 + wt * 64 + ti * 16 + r;
        if (tok >= rows) continue;
        const float s_tok = sa[tok];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int ch = c0 + wm * 64 + mi * 16 + 4 * g;
            if (ch >= n) continue;
            const float4 s_ch = *reinterpret_cast<const float4*>(sw + ch);
            float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (bias) b = *reinterpret_cast<const float4*>(bias + ch);
            float o[4] = {(float)acc[mi][ti][0] * s_tok * s_ch.x + b.x, (float)acc[mi][ti][1] * s_tok * s_ch.y + b.y,
                          (float)acc[mi][ti][2] * s_tok * s_ch.z + b.z, (float)acc[mi][ti][3] * s_tok * s_ch.w + b.w};
            const long at = tok * n + ch;
            if (res) {
                const v2u rv = *reinterpret_cast<const v2u*>(res + at);
                o[0] += half_to_f32<BF>((unsigned short)(rv.x & 0xffffu));
                o[1] += half_to_f32<BF>((unsigned short)(rv.x >> 16));
                o[2] += half_to_f32<BF>((unsigned short)(rv.y & 0xffffu));
                o[3] += half_to_f32<BF>((unsigned short)(rv.y >> 16));
            }
            v2u ov;
            ov.x = (unsigned)f32_to_half<BF>(o[0]) | ((unsigned)f32_to_half<BF>(o[1]) << 16);
            ov.y = (unsigned)f32_to_half<BF>(o[2]) | ((unsigned)f32_to_half<BF>(o[3]) << 16);
            *reinterpret_cast<v2u*>(y + at) = ov;
        }
    }
}

// ---- quantising one row ---------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// the larger of two magnitudes; a NaN on either side stays (fmaxf would drop it)
__device__ __forceinline__ float max_nan(float a, float b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ float wave_max_nan(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max_nan(v, __shfl_xor(v, m, 64));
    return v;
}

// (inv, s) of a row with largest magnitude amax: two correctly rounded float32 divisions; an all-zero row keeps scale 1.  A NaN
// amax gives inv = s = NaN, an infinite one inv = 0 and s = inf.
__device__ __forceinline__ void row_scales(float amax, float& inv, float& s) {
    inv = amax == 0.0f ? 1.0f : I8_MAX / amax;
    s = amax == 0.0f ? 1.0f : amax / I8_MAX;
}

// one code, as the low byte of an unsigned: round to nearest even, a NaN -> 0, clamped to +-127
__device__ __forceinline__ unsigned code_i8(float x) {
    float q = rintf(x);
    q = q != q ? 0.0f : q;
    q = fminf(fmaxf(q, -I8_MAX), I8_MAX);
    return (unsigned)(int)q & 0xffu;
}

__device__ __forceinline__ v2u codes8(const float (&f)[8], float inv) {
    unsigned c[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = code_i8(f[j] * inv);
    v2u o;
    o.x = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    o.y = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
    return o;
}

template <bool BF>
__device__ __forceinline__ void unpack8(const v4u& v, float (&f)[8]) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = half_to_f32<BF>((unsigned short)(w[i] & 0xffffu));
        f[2 * i + 1] = half_to_f32<BF>((unsigned short)(w[i] >> 16));
    }
}
__device__ __forceinline__ void load8_f32(const float* p, float (&f)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
}

// silu(t) = t / (1 + exp(-t)) through exp(-|t|), as swiglu_rows_h_kernel evaluates it (no exponential overflows)
__device__ __forceinline__ float silu_f32(float t) {
    const float e = expf(-fabsf(t));
    const float num = t >= 0.0f ? t : t * e;
    return num / (1.0f + e);
}

// The row's float32 values are in f (this lane's vectors lane + 64 i, below cv): the row maximum over the wave, then the codes as
// one 8-byte store per vector and the scale from lane 0.
template <int VPL>
__device__ __forceinline__ void quantise_row(const float (&f)[VPL][8], int lane, int cv, signed char* qrow, float* srow) {
    float amax = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int j = 0; j < 8; ++j) amax = max_nan(amax, fabsf(f[i][j]));
        }
    amax = wave_max_nan(amax);
    float inv, s;
    row_scales(amax, inv, s);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) *reinterpret_cast<v2u*>(qrow + 8 * v) = codes8(f[i], inv);
    }
    if (lane == 0) *srow = s;
}

// One wave per row, the row in registers (layernorm_rows_h_kernel's form and arithmetic: the mean, then the variance of the centred
// values, the affine as one fmaf), four rows per workgroup; what would be rounded to half there is quantised here.
template <bool BF, int VPL>
__global__ __launch_bounds__(ET) void layernorm_rows_qi8_kernel(const unsigned short* __restrict__ x, long stride, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps, long rows, int c,
                                                                 signed char* __restrict__ q, float* __restrict__ s) {
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
            for (int j = 0; j < 8; ++j) sum += f[i][j];
        }
    }
    const float mean = wave_sum(sum) / (float)c;
    float sq = 0.0f;
#pragma unroll
    for (int i = 0; i < VPL; ++i)
        if (lane + 64 * i < cv) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                f[i][j] -= mean;
                sq = fmaf(f[i][j], f[i][j], sq);
            }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)c + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            float gm[8], bt[8];
            load8_f32(gamma + 8 * v, gm);
            load8_f32(beta + 8 * v, bt);
#pragma unroll
            for (int j = 0; j < 8; ++j) f[i][j] = fmaf(f[i][j] * rstd, gm[j], bt[j]);
        }
    }
    quantise_row<VPL>(f, lane, cv, q + row * (long)c, s + row);
}

// The activation between fc1 and fc2, one wave per row of `hidden` outputs.  SWIGLU: the input row is [gate H | value H].
template <bool BF, bool SWIGLU, int VPL>
__global__ __launch_bounds__(ET) void act_rows_qi8_kernel(const unsigned short* __restrict__ x, long rows, int hidden,
                                                           signed char* __restrict__ q, float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int cv = hidden >> 3;
    const unsigned short* xr = x + row * (SWIGLU ? 2L : 1L) * hidden;
    float f[VPL][8];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int v = lane + 64 * i;
        if (v < cv) {
            unpack8<BF>(*reinterpret_cast<const v4u*>(xr + 8 * v), f[i]);
            if constexpr (SWIGLU) {
                float val[8];
                unpack8<BF>(*reinterpret_cast<const v4u*>(xr + hidden + 8 * v), val);
#pragma unroll
                for (int j = 0; j < 8; ++j) f[i][j] = silu_f32(f[i][j]) * val[j];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) f[i][j] = 0.5f * f[i][j] * (1.0f + erff(f[i][j] * 0.70710678118654752440f));
            }
        }
    }
    quantise_row<VPL>(f, lane, cv, q + row * (long)hidden, s + row);
}

// Weights: one wave per output channel, the row read twice (the maximum, then the codes; the second read is served by the cache --
// this runs once per layer, in `prepare`).  k % 4 == 0.
__global__ __launch_bounds__(ET) void linear_int8_pack_weights_kernel(const float* __restrict__ w, long n, int k, signed char* __restrict__ q,
                                                                       float* __restrict__ s) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (ET / 64) + (threadIdx.x >> 6);
    if (row >= n) return;
    const float4* wr = reinterpret_cast<const float4*>(w + row * (long)k);
    float amax = 0.0f;
    for (int v = lane; v < k / 4; v += 64) {
        const float4 t = wr[v];
        amax = max_nan(max_nan(amax, max_nan(fabsf(t.x), fabsf(t.y))), max_nan(fabsf(t.z), fabsf(t.w)));
    }
    amax = wave_max_nan(amax);
    float inv, sc;
    row_scales(amax, inv, sc);
    unsigned* qr = reinterpret_cast<unsigned*>(q + row * (long)k);
    for (int v = lane; v < k / 4; v += 64) {
        const float4 t = wr[v];
        qr[v] = code_i8(t.x * inv) | (code_i8(t.y * inv) << 8) | (code_i8(t.z * inv) << 16) | (code_i8(t.w * inv) << 24);
    }
    if (lane == 0) s[row] = sc;
}

bool misaligned(std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 15) != 0;
}

// the shapes the GEMM takes: 0, or the error code of everything else
int linear_int8_shape(int64_t rows, int64_t n, int64_t k) {
    if (rows <= 0 || n <= 0 || k <= 0) return TIA_EINVAL;
    if (k % 128 != 0 || n % 16 != 0 || k > K_MAX || n > (1 << 24)) return TIA_ESIZE;
    const int64_t tiles = ((rows + BT - 1) / BT) * ((n + BT - 1) / BT);
    if (rows > (int64_t(1) << 40) || tiles > 0x7fffffffL) return TIA_ESIZE;
    return TIA_OK;
}

}  // namespace

extern "C" int tia_linear_int8_serves(int64_t rows, int64_t n, int64_t k) {
    const int rc = linear_int8_shape(rows, n, k);
    return rc == TIA_OK ? 1 : (rc == TIA_ESIZE ? 0 : rc);
}

extern "C" int tia_linear_int8_rows(const void* d_a, const float* d_sa, const void* d_w, const float* d_sw, const float* d_bias,
                                    const void* d_residual, void* d_y, int64_t rows, int64_t n, int64_t k, int32_t dtype, void* stream) {
    if (!d_a || !d_sa || !d_w || !d_sw || !d_y) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    const int rc = linear_int8_shape(rows, n, k);
    if (rc != TIA_OK) return rc;
    if (misaligned({d_a, d_sa, d_w, d_sw, d_bias, d_residual, d_y})) return TIA_EINVAL;
    const int n_ct = (int)((n + BT - 1) / BT);
    const dim3 grid((unsigned)(((rows + BT - 1) / BT) * n_ct));
    const auto kernel = dtype == TIA_DT_BF16 ? linear_int8_rows_kernel<true> : linear_int8_rows_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(ET), 0, (hipStream_t)stream, static_cast<const signed char*>(d_a), d_sa,
                       static_cast<const signed char*>(d_w), d_sw, d_bias, static_cast<const unsigned short*>(d_residual),
                       static_cast<unsigned short*>(d_y), (long)rows, (int)n, (int)k, n_ct);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_linear_int8_pack_weights(const float* d_w, int64_t n, int64_t k, void* d_q, float* d_scale, void* stream) {
    if (!d_w || !d_q || !d_scale) return TIA_EINVAL;
    const int rc = linear_int8_shape(1, n, k);
    if (rc != TIA_OK) return rc;
    if (misaligned({d_w, d_q, d_scale})) return TIA_EINVAL;
    const dim3 grid((unsigned)((n + ET / 64 - 1) / (ET / 64)));
    hipLaunchKernelGGL(linear_int8_pack_weights_kernel, grid, dim3(ET), 0, (hipStream_t)stream, d_w, (long)n, (int)k,
                       static_cast<signed char*>(d_q), d_scale);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_layernorm_rows_qi8(const void* d_x, int64_t row_stride, const float* d_gamma, const float* d_beta, float eps, void* d_q,
                                      float* d_scale, int64_t rows, int64_t c, int32_t dtype, void* stream) {
    if (!d_x || !d_gamma || !d_beta || !d_q || !d_scale || rows <= 0 || c <= 0 || !(eps >= 0.0f)) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((c & 15) != 0 || c > 8192) return TIA_ESIZE;
    if (row_stride < c || (row_stride & 7) != 0) return TIA_EINVAL;
    if (misaligned({d_x, d_gamma, d_beta, d_q, d_scale})) return TIA_EINVAL;
    const long blocks = (rows + ET / 64 - 1) / (ET / 64);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    const int vpl = (int)((c / 8 + 63) / 64);
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    const unsigned short* x = static_cast<const unsigned short*>(d_x);
    signed char* q = static_cast<signed char*>(d_q);
#define TIA_LNQ(BF, V) \
    hipLaunchKernelGGL((layernorm_rows_qi8_kernel<BF, V>), grid, dim3(ET), 0, st, x, (long)row_stride, d_gamma, d_beta, eps, (long)rows, (int)c, q, d_scale)
#define TIA_LNQ_V(BF)                     \
    do {                                  \
        if (vpl <= 1) TIA_LNQ(BF, 1);      \
        else if (vpl <= 2) TIA_LNQ(BF, 2); \
        else if (vpl <= 4) TIA_LNQ(BF, 4); \
        else if (vpl <= 8) TIA_LNQ(BF, 8); \
        else TIA_LNQ(BF, 16);              \
    } while (0)
    if (dtype == TIA_DT_BF16) TIA_LNQ_V(true);
    else TIA_LNQ_V(false);
#undef TIA_LNQ_V
#undef TIA_LNQ
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

namespace {

template <bool SWIGLU>
int act_rows_qi8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    if (!d_x || !d_q || !d_scale || rows <= 0 || hidden <= 0) return TIA_EINVAL;
    if (dtype != TIA_DT_F16 && dtype != TIA_DT_BF16) return TIA_EINVAL;
    if ((hidden & 15) != 0 || hidden > 8192) return TIA_ESIZE;
    if (misaligned({d_x, d_q, d_scale})) return TIA_EINVAL;
    const long blocks = (rows + ET / 64 - 1) / (ET / 64);
    if (blocks > 0x7fffffffL) return TIA_ESIZE;
    const int vpl = (int)((hidden / 8 + 63) / 64);
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    const unsigned short* x = static_cast<const unsigned short*>(d_x);
    signed char* q = static_cast<signed char*>(d_q);
#define TIA_ACTQ(BF, V) \
    hipLaunchKernelGGL((act_rows_qi8_kernel<BF, SWIGLU, V>), grid, dim3(ET), 0, st, x, (long)rows, (int)hidden, q, d_scale)
#define TIA_ACTQ_V(BF)                     \
    do {                                   \
        if (vpl <= 1) TIA_ACTQ(BF, 1);      \
        else if (vpl <= 2) TIA_ACTQ(BF, 2); \
        else if (vpl <= 4) TIA_ACTQ(BF, 4); \
        else if (vpl <= 8) TIA_ACTQ(BF, 8); \
        else TIA_ACTQ(BF, 16);              \
    } while (0)
    if (dtype == TIA_DT_BF16) TIA_ACTQ_V(true);
    else TIA_ACTQ_V(false);
#undef TIA_ACTQ_V
#undef TIA_ACTQ
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

}  // namespace

extern "C" int tia_gelu_rows_qi8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    return act_rows_qi8<false>(d_x, d_q, d_scale, rows, hidden, dtype, stream);
}

extern "C" int tia_swiglu_rows_qi8(const void* d_x, void* d_q, float* d_scale, int64_t rows, int64_t hidden, int32_t dtype, void* stream) {
    return act_rows_qi8<true>(d_x, d_q, d_scale, rows, hidden, dtype, stream);
}
