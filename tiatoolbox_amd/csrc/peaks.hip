// Peak detection on probability maps: skimage.feature.peak_local_max with a square footprint, p_norm = inf and no labels, as
// tiatoolbox_amd/utils/_peaks.py states it (the statement is the contract).  The device part of one call:
//
//   1. peak_minmax_kernel      per-plane minimum and maximum (order-preserving integer keys, atomicMin / atomicMax: the result
//                              of a minimum does not depend on the order of its operands)
//   2. peak_window_kernel<Max> the (2d+1)^2 window maximum on an LDS tile with a halo of d pixels, edge-replicated, separable
//                              (rows, then columns) and exact; the epilogue writes the candidate flag: value == window maximum,
//                              plane not constant, value > threshold (strict), outside the excluded border
//   3. peak_window_kernel<Sum> the number of candidates in the (2d-1)^2 window around every candidate, same tile code on the
//                              flag plane with zeros outside the plane; two or more = "contested": another candidate lies at
//                              Chebyshev distance < d.  state = 0 none / 1 candidate / 2 contested candidate
//   4. peak_count_kernel, peak_offsets_kernel, peak_write_kernel: count per raster chunk, exclusive prefix sum per plane, then
//      (y, x, value, contested) of every candidate in raster order -- the count pass followed by a write pass of
//      tia_hover_contour_scan / _write: no order-dependent atomics.
//
// Two candidates at Chebyshev distance <= d have equal values (each is the maximum of a window that holds the other), so the
// statement's greedy spacing walk only ever decides between equal values, in raster order, and only among contested candidates.
// tia_peak_resolve_host is that walk on the host over the contested set alone (one sweep with the last accepted row per column).
//
// NaN is outside the domain (the result is then unspecified; every access stays in bounds: no index depends on a value);
// +-inf and +-0 are inside it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "common.hpp"

namespace {

constexpr int PEAK_TILE = 32;        // output tile side; the LDS tile is (PEAK_TILE + 2 r)^2 with r the window radius
constexpr int PEAK_THREADS = 256;
constexpr int PEAK_MAX_DISTANCE = 64;
constexpr int PEAK_CHUNK_ITEMS = 8;  // consecutive pixels per thread of the count / write passes
constexpr int PEAK_CHUNK = PEAK_THREADS * PEAK_CHUNK_ITEMS;

// order-preserving map float32 -> uint32 (-0 < +0), and back
__device__ __forceinline__ unsigned f32_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

__global__ void peak_minmax_init_kernel(unsigned* __restrict__ keys, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        keys[2 * i] = 0xffffffffu;
        keys[2 * i + 1] = 0u;
    }
}

// grid = (blocks per plane, planes in this launch); keys [n][2] = key of the minimum, key of the maximum
__global__ __launch_bounds__(PEAK_THREADS) void peak_minmax_kernel(const float* __restrict__ img, long hw,
                                                                   unsigned* __restrict__ keys) {
    const float* p = img + (size_t)blockIdx.y * (size_t)hw;
    unsigned lo = 0xffffffffu, hi = 0u;
    for (long i = (long)blockIdx.x * PEAK_THREADS + threadIdx.x; i < hw; i += (long)gridDim.x * PEAK_THREADS) {
        const unsigned k = f32_key(p[i]);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = __shfl_down(lo, o, 64), b = __shfl_down(hi, o, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&keys[2 * (size_t)blockIdx.y], lo);
        atomicMax(&keys[2 * (size_t)blockIdx.y + 1], hi);
    }
}

struct PeakThreshold {
    float abs_value, rel_value;
    int has_abs, has_rel, border;
};

// Window maximum of the float32 planes; the epilogue decides the candidate flag.
struct MaxOp {
    using V = float;
    const float* img;
    const unsigned* keys;
    uint8_t* flags;
    PeakThreshold thr;
    __device__ V load(size_t plane, int y, int x, int h, int w) const {  // mode="nearest": the edge pixel repeats
        y = y < 0 ? 0 : (y >= h ? h - 1 : y);
        x = x < 0 ? 0 : (x >= w ? w - 1 : x);
        return img[plane * (size_t)h * w + (size_t)y * w + x];
    }
    __device__ static V join(V a, V b) { return b > a ? b : a; }
    __device__ void store(size_t plane, int y, int x, int h, int w, V window, V centre) const {
        const float mn = key_f32(keys[2 * plane]), mx = key_f32(keys[2 * plane + 1]);
        float t = thr.has_abs ? thr.abs_value : mn;
        if (thr.has_rel) {
            const float tr = thr.rel_value * mx;
            if (tr > t) t = tr;
        }
        const bool single = (long)h * w == 1;
        bool cand = centre > t && (single || (centre == window && !(mn == mx)));
        const int b = thr.border;
        if (y < b || x < b || y >= h - b || x >= w - b) cand = false;
        flags[plane * (size_t)h * w + (size_t)y * w + x] = cand ? 1 : 0;
    }
};

// Number of candidate flags in the window (zeros outside the plane); the epilogue writes the candidate's state.
struct SumOp {
    using V = int;
    const uint8_t* flags;
    uint8_t* state;
    __device__ V load(size_t plane, int y, int x, int h, int w) const {
        if ((unsigned)y >= (unsigned)h || (unsigned)x >= (unsigned)w) return 0;
        return flags[plane * (size_t)h * w + (size_t)y * w + x];
    }
    __device__ static V join(V a, V b) { return a + b; }
    __device__ void store(size_t plane, int y, int x, int h, int w, V window, V centre) const {
        state[plane * (size_t)h * w + (size_t)y * w + x] = centre ? (window >= 2 ? 2 : 1) : 0;
    }
};

// One workgroup = one PEAK_TILE^2 output tile of one plane.  LDS: a [S][S] (the tile with its halo), b [S][PEAK_TILE] (row
// reductions), S = PEAK_TILE + 2 r.  Consecutive lanes read consecutive LDS words in both passes: no bank conflicts.
template <class Op>
__global__ __launch_bounds__(PEAK_THREADS) void peak_window_kernel(Op op, int h, int w, int r, int tiles_x, int tiles_per_plane) {
    using V = typename Op::V;
    extern __shared__ __attribute__((aligned(16))) unsigned char peak_smem[];
    const int S = PEAK_TILE + 2 * r;
    V* a = reinterpret_cast<V*>(peak_smem);
    V* b = a + S * S;
    const size_t plane = blockIdx.x / (unsigned)tiles_per_plane;
    const int t = (int)(blockIdx.x - plane * (unsigned)tiles_per_plane);
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int y0 = ty * PEAK_TILE - r, x0 = tx * PEAK_TILE - r;
    const int rows = min(PEAK_TILE, h - ty * PEAK_TILE);  // output rows of this tile that lie in the plane
    const int srows = rows + 2 * r;                        // LDS rows they read
    for (int i = threadIdx.x; i < srows * S; i += PEAK_THREADS) {
        const int yy = i / S, xx = i - yy * S;
        a[i] = op.load(plane, y0 + yy, x0 + xx, h, w);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < srows * PEAK_TILE; i += PEAK_THREADS) {
        const int yy = i / PEAK_TILE, xo = i - yy * PEAK_TILE;
        const V* row = a + yy * S + xo;
        V m = row[0];
        for (int k = 1; k <= 2 * r; ++k) m = Op::join(m, row[k]);
        b[i] = m;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * PEAK_TILE; i += PEAK_THREADS) {
        const int yo = i / PEAK_TILE, xo = i - yo * PEAK_TILE;
        const int x = tx * PEAK_TILE + xo;
        if (x >= w) continue;
        const V* col = b + yo * PEAK_TILE + xo;
        V m = col[0];
        for (int k = 1; k <= 2 * r; ++k) m = Op::join(m, col[k * PEAK_TILE]);
        op.store(plane, ty * PEAK_TILE + yo, x, h, w, m, a[(yo + r) * S + xo + r]);
    }
}

// counts [n][chunks]: candidates in each chunk of PEAK_CHUNK consecutive pixels of a plane; grid = n * chunks
__global__ __launch_bounds__(PEAK_THREADS) void peak_count_kernel(const uint8_t* __restrict__ state, long hw, long chunks,
                                                                  int* __restrict__ counts) {
    __shared__ int part[PEAK_THREADS / 64];
    const size_t plane = blockIdx.x / (unsigned long)chunks;
    const long chunk = (long)(blockIdx.x - plane * (unsigned long)chunks);
    const uint8_t* s = state + plane * (size_t)hw;
    const long lo = chunk * PEAK_CHUNK + (long)threadIdx.x * PEAK_CHUNK_ITEMS;
    int c = 0;
#pragma unroll
    for (int k = 0; k < PEAK_CHUNK_ITEMS; ++k)
        if (lo + k < hw && s[lo + k] != 0) ++c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int k = 0; k < PEAK_THREADS / 64; ++k) total += part[k];
        counts[blockIdx.x] = total;
    }
}

// per plane (one workgroup each): counts -> exclusive prefix sum in place, totals[plane] = the plane's candidates
__global__ __launch_bounds__(1024) void peak_offsets_kernel(int* __restrict__ counts, long chunks, long long* __restrict__ totals) {
    __shared__ long long part[1024];
    int* c = counts + (size_t)blockIdx.x * (size_t)chunks;
    const int t = threadIdx.x;
    const long per = (chunks + 1023) / 1024;
    const long lo = (long)t * per < chunks ? (long)t * per : chunks, hi = lo + per < chunks ? lo + per : chunks;
    long long s = 0;
    for (long i = lo; i < hi; ++i) s += c[i];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - s;
    for (long i = lo; i < hi; ++i) {
        const int n = c[i];
        c[i] = (int)run;  // a plane has fewer than 2^31 pixels
        run += n;
    }
    if (t == 1023) totals[blockIdx.x] = part[1023];
}

// candidate j of plane p (raster order) goes to row bases[p] + j of yx [capacity][2], value [capacity], contested [capacity]
__global__ __launch_bounds__(PEAK_THREADS) void peak_write_kernel(const float* __restrict__ img, const uint8_t* __restrict__ state,
                                                                  long hw, int w, long chunks, const int* __restrict__ offsets,
                                                                  const long long* __restrict__ bases, long long capacity,
                                                                  int* __restrict__ yx, float* __restrict__ value,
                                                                  uint8_t* __restrict__ contested) {
    __shared__ int part[PEAK_THREADS / 64];
    const size_t plane = blockIdx.x / (unsigned long)chunks;
    const long chunk = (long)(blockIdx.x - plane * (unsigned long)chunks);
    const uint8_t* s = state + plane * (size_t)hw;
    const long lo = chunk * PEAK_CHUNK + (long)threadIdx.x * PEAK_CHUNK_ITEMS;
    uint8_t st[PEAK_CHUNK_ITEMS];
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < PEAK_CHUNK_ITEMS; ++k) {
        st[k] = lo + k < hw ? s[lo + k] : 0;
        if (st[k] != 0) ++c;
    }
    const unsigned incl = tia::wave_incl_scan_u32(c);
    if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = (int)incl;
    __syncthreads();
    long long at = bases[plane] + offsets[blockIdx.x] + (incl - c);
    for (int k = 0; k < (int)(threadIdx.x >> 6); ++k) at += part[k];
#pragma unroll
    for (int k = 0; k < PEAK_CHUNK_ITEMS; ++k) {
        if (st[k] == 0) continue;
        if (at >= 0 && at < capacity) {
            const long p = lo + k;
            const int y = (int)(p / w);
            yx[2 * at] = y;
            yx[2 * at + 1] = (int)(p - (long)y * w);
            value[at] = img[plane * (size_t)hw + p];
            contested[at] = st[k] == 2 ? 1 : 0;
        }
        ++at;
    }
}

size_t window_lds_bytes(int r, size_t elem) {
    const size_t s = PEAK_TILE + 2 * (size_t)r;
    return (s * s + s * PEAK_TILE) * elem;
}

tia::DeviceOnce g_peak_lds_once;

bool peak_lds_setup() {
    const int bytes = (int)window_lds_bytes(PEAK_MAX_DISTANCE, 4);  // 122,880 of the CU's 163,840 bytes
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&peak_window_kernel<MaxOp>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               bytes) == hipSuccess &&
           hipFuncSetAttribute(reinterpret_cast<const void*>(&peak_window_kernel<SumOp>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               bytes) == hipSuccess;
}

int check_planes(int64_t n, int64_t h, int64_t w) {
    if (n <= 0 || h <= 0 || w <= 0) return TIA_EINVAL;
    if (h > 0x7fffffffLL || w > 0x7fffffffLL || h * w > 0x7fffffffLL) return TIA_ESIZE;
    return TIA_OK;
}

}  // namespace

extern "C" size_t tia_peak_chunks(int64_t h, int64_t w) {
    if (check_planes(1, h, w) != TIA_OK) return 0;
    return (size_t)((h * w + PEAK_CHUNK - 1) / PEAK_CHUNK);
}

extern "C" int tia_peak_scan_f32(const float* d_image, int64_t n, int64_t h, int64_t w, int32_t min_distance,
                                 int32_t has_threshold_abs, float threshold_abs, int32_t has_threshold_rel, float threshold_rel,
                                 int32_t border, uint32_t* d_minmax, uint8_t* d_flags, uint8_t* d_state, int32_t* d_offsets,
                                 int64_t* d_totals, void* stream) {
    if (!d_image || !d_minmax || !d_flags || !d_state || !d_offsets || !d_totals || border < 0) return TIA_EINVAL;
    const int rc = check_planes(n, h, w);
    if (rc != TIA_OK) return rc;
    if (min_distance < 1 || min_distance > PEAK_MAX_DISTANCE) return TIA_ESIZE;
    const long hw = (long)(h * w);
    const long tiles_x = (w + PEAK_TILE - 1) / PEAK_TILE, tiles_y = (h + PEAK_TILE - 1) / PEAK_TILE;
    const long tiles = tiles_x * tiles_y, chunks = (hw + PEAK_CHUNK - 1) / PEAK_CHUNK;
    if (tiles > 0x7fffffffL / n || chunks > 0x7fffffffL / n) return TIA_ESIZE;  // one grid dimension carries plane * tile
    if (!g_peak_lds_once.ensure(peak_lds_setup)) return TIA_ELAUNCH;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(peak_minmax_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_minmax, (long)n);
    long mm_blocks = (hw + PEAK_THREADS * 16L - 1) / (PEAK_THREADS * 16L);
    if (mm_blocks > 2048) mm_blocks = 2048;
    for (int64_t p0 = 0; p0 < n; p0 += 65535) {  // grid.y carries the plane
        const int64_t np = n - p0 < 65535 ? n - p0 : 65535;
        hipLaunchKernelGGL(peak_minmax_kernel, dim3((unsigned)mm_blocks, (unsigned)np), dim3(PEAK_THREADS), 0, st,
                           d_image + (size_t)p0 * hw, hw, d_minmax + 2 * p0);
    }
    const PeakThreshold thr{threshold_abs, threshold_rel, has_threshold_abs != 0, has_threshold_rel != 0, border};
    hipLaunchKernelGGL(peak_window_kernel<MaxOp>, dim3((unsigned)(n * tiles)), dim3(PEAK_THREADS),
                       window_lds_bytes(min_distance, sizeof(float)), st, MaxOp{d_image, d_minmax, d_flags, thr}, (int)h, (int)w,
                       (int)min_distance, (int)tiles_x, (int)tiles);
    // at min_distance 1 the strict spacing test can reject nothing: the window is the candidate itself
    hipLaunchKernelGGL(peak_window_kernel<SumOp>, dim3((unsigned)(n * tiles)), dim3(PEAK_THREADS),
                       window_lds_bytes(min_distance - 1, sizeof(int)), st, SumOp{d_flags, d_state}, (int)h, (int)w,
                       (int)min_distance - 1, (int)tiles_x, (int)tiles);
    hipLaunchKernelGGL(peak_count_kernel, dim3((unsigned)(n * chunks)), dim3(PEAK_THREADS), 0, st, d_state, hw, chunks, d_offsets);
    hipLaunchKernelGGL(peak_offsets_kernel, dim3((unsigned)n), dim3(1024), 0, st, d_offsets, chunks, (long long*)d_totals);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_peak_write_f32(const float* d_image, const uint8_t* d_state, int64_t n, int64_t h, int64_t w,
                                  const int32_t* d_offsets, const int64_t* d_bases, int64_t capacity, int32_t* d_yx,
                                  float* d_value, uint8_t* d_contested, void* stream) {
    if (!d_image || !d_state || !d_offsets || !d_bases || capacity < 0) return TIA_EINVAL;
    const int rc = check_planes(n, h, w);
    if (rc != TIA_OK) return rc;
    if (capacity == 0) return TIA_OK;
    if (!d_yx || !d_value || !d_contested) return TIA_EINVAL;
    const long hw = (long)(h * w), chunks = (hw + PEAK_CHUNK - 1) / PEAK_CHUNK;
    if (chunks > 0x7fffffffL / n) return TIA_ESIZE;
    hipLaunchKernelGGL(peak_write_kernel, dim3((unsigned)(n * chunks)), dim3(PEAK_THREADS), 0, (hipStream_t)stream, d_image,
                       d_state, hw, (int)w, chunks, d_offsets, (const long long*)d_bases, (long long)capacity, d_yx, d_value,
                       d_contested);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_peak_resolve_host(const int32_t* yx, int64_t k, int64_t w, int32_t min_distance, uint8_t* accept) {
    if (k < 0 || w <= 0 || w > 0x7fffffffLL || min_distance < 1) return TIA_EINVAL;
    if (k == 0) return TIA_OK;
    if (!yx || !accept) return TIA_EINVAL;
    const long long never = -(1LL << 40);
    std::vector<long long> last((size_t)w, never);  // per column: the row of the candidate accepted last
    const long long d = min_distance;
    long long py = -1, px = -1;
    for (int64_t i = 0; i < k; ++i) {
        const long long y = yx[2 * i], x = yx[2 * i + 1];
        if (y < 0 || x < 0 || x >= w || y < py || (y == py && x <= px)) return TIA_EINVAL;  // raster order, inside the plane
        py = y;
        px = x;
        const long long lo = x - d + 1 > 0 ? x - d + 1 : 0, hi = x + d - 1 < w - 1 ? x + d - 1 : w - 1;
        bool ok = true;
        for (long long c = lo; c <= hi; ++c)
            if (y - last[(size_t)c] < d) {
                ok = false;
                break;
            }
        if (ok) last[(size_t)x] = y;
        accept[i] = ok ? 1 : 0;
    }
    return TIA_OK;
}
