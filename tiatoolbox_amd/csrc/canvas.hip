// Overlap-average stitching of patch probabilities into a whole-slide canvas on gfx950.
// Reference: models/engine/semantic_segmentor.py:1141-1263 (merge_batch_to_canvas / merge_horizontal),
// :1398-1534 (merge_vertical_chunkwise), patch_predictor.py:382-446 (argmax).
// Gather formulation: one thread owns one canvas element and sums its (<= a few) contributing blocks in
// the reference's order, so results are deterministic and bit-identical to the NumPy path -- no float atomics.
// Also here: merge_patch_rects_kernel, the patch classifier's merge_predictions (models/engine/patch_predictor.py:merge_predictions
// of the reference: `out[y0:y1, x0:x1] += p[i]` in a loop over patches, then a divide by the coverage count and an argmax): one
// workgroup per map tile walks the tile's ascending list of patch rectangles, so every pixel adds its patches in patch order;
// merge_patch_grids_kernel, the same walk for merge_attention, where a patch brings a grid of attention cells that every covered
// pixel samples (nearest or bilinear) instead of one row of values;
// and the batched patch reads of the WSI engines (plain, area-resampled, bicubic) further down.
#include <float.h>

#include "common.hpp"

#pragma clang fp contract(off)

namespace tia {

constexpr int CT = 256;

__global__ __launch_bounds__(CT) void block_flags_kernel(const float* __restrict__ blocks, long per_block, int* __restrict__ flags) {
    // flags[b] = any(block b != 0)
    const float* p = blocks + (size_t)blockIdx.y * per_block;
    int any = 0;
    for (long i = (long)blockIdx.x * CT + threadIdx.x; i < per_block; i += (long)gridDim.x * CT) any |= (p[i] != 0.0f);
    if (__ballot(any) != 0ull && lane_id() == 0) atomicOr(&flags[blockIdx.y], 1);
}

__global__ __launch_bounds__(CT) void row_merge_kernel(const float* __restrict__ blocks, const int* __restrict__ xs,
                                                        const int* __restrict__ flags, int n, int oh, int ow, int c, int width,
                                                        float* __restrict__ row, uint8_t* __restrict__ cnt) {
    const long total = (long)oh * width;
    for (long i = (long)blockIdx.x * CT + threadIdx.x; i < total; i += (long)gridDim.x * CT) {
        const int y = (int)(i / width), x = (int)(i - (long)y * width);
        float acc[8];
        for (int k = 0; k < c; ++k) acc[k] = 0.0f;
        unsigned count = 0;
        for (int b = 0; b < n; ++b) {
            const int x0 = xs[b];
            if (x < x0 || x >= x0 + ow || !flags[b]) continue;
            const float* src = blocks + (((size_t)b * oh + y) * ow + (x - x0)) * c;
            for (int k = 0; k < c; ++k) acc[k] = acc[k] + src[k];
            ++count;
        }
        float* dst = row + (size_t)i * c;
        for (int k = 0; k < c; ++k) dst[k] = acc[k];
        cnt[i] = (uint8_t)count;
    }
}

__global__ __launch_bounds__(CT) void finalize_kernel(const float* __restrict__ row_a, const uint8_t* __restrict__ cnt_a, long ys_a,
                                                       const float* __restrict__ row_b, const uint8_t* __restrict__ cnt_b, long ys_b,
                                                       int oh, int width, int c, long y_begin, long y_end,
                                                       float* __restrict__ probs, uint8_t* __restrict__ pred) {
    const long total = (y_end - y_begin) * width;
    for (long i = (long)blockIdx.x * CT + threadIdx.x; i < total; i += (long)gridDim.x * CT) {
        const long y = y_begin + i / width;
        const int x = (int)(i % width);
        const long ya = y - ys_a;
        const bool has_a = ya >= 0 && ya < oh;
        const long yb = y - ys_b;
        const bool has_b = row_b != nullptr && yb >= 0 && yb < oh;
        unsigned count = (has_a ? cnt_a[ya * width + x] : 0u) + (has_b ? cnt_b[yb * width + x] : 0u);
        count = (uint8_t)count;          // numpy uint8 arithmetic
        const float denom = (float)(count == 0 ? 1u : count);
        int best = 0;
        float bestv = 0.0f;
        for (int k = 0; k < c; ++k) {
            float v = has_a ? row_a[((size_t)ya * width + x) * c + k] : 0.0f;
            if (has_b) v = v + row_b[((size_t)yb * width + x) * c + k];
            v = v / denom;
            if (probs) probs[((size_t)y * width + x) * c + k] = v;
            // np.argmax: the first NaN wins, else the first maximum (a NaN, once held, is never replaced: both tests are false)
            if (k == 0 || v > bestv || (v != v && bestv == bestv)) {
                bestv = v;
                best = k;
            }
        }
        pred[(size_t)y * width + x] = (uint8_t)best;
    }
}


// ---- merge_predictions: per-patch class rows painted into a whole-slide map ---------------------------------------------
// sum[Y, X, k] = the float32 sum of values[i, k] over the patches i whose map-space rectangle (x0, y0, x1, y1; half-open)
// holds (Y, X), added one at a time in ascending i; count[Y, X] = how many.  A workgroup owns one tile_h x tile_w tile of the
// map and walks the tile's list (every patch whose rectangle meets the tile, ascending: the order is the contract); the list
// item, its rectangle and its row of values are the same for every lane of a wave, so they come through scalar loads and
// the per-pixel work is a coverage test and up to kMergeChunk adds into registers.  More classes than kMergeChunk take further
// passes over the list, the order within a class unchanged.  raw = float32(float64(sum) / (float64(count) + 1e-8)) (the
// reference's divisor); label = 1 + the first maximum of the SUMS where count > 0 (one positive divisor per pixel: the argmax
// of the exact quotient, whatever the quotient's rounding), 0 elsewhere.  A tile larger than the workgroup takes several
// pixels per thread.  List items outside [0, n) are skipped, so a bad list cannot read outside `values`.
constexpr int kMergeChunk = 16;

template <typename L>
__global__ __launch_bounds__(CT) void merge_patch_rects_kernel(const int* __restrict__ rects, const float* __restrict__ values, int n,
                                                                int c, int h, int w, const int* __restrict__ tile_offsets,
                                                                const int* __restrict__ tile_items, int tile_h, int tile_w,
                                                                int tiles_x, float* __restrict__ sum, float* __restrict__ raw,
                                                                int* __restrict__ count, L* __restrict__ labels) {
    const int tile = (int)blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * tile_h, x0 = tx * tile_w;
    const int th = min(tile_h, h - y0), tw = min(tile_w, w - x0);
    const int lb = tile_offsets[tile], le = tile_offsets[tile + 1];
    for (int p = threadIdx.x; p < th * tw; p += CT) {
        const int py = p / tw;
        const int X = x0 + (p - py * tw), Y = y0 + py;
        const size_t pix = (size_t)Y * w + X;
        int best = 0, cnt = 0;
        float bestv = 0.0f;
        for (int c0 = 0; c0 < c; c0 += kMergeChunk) {
            const int cc = min(kMergeChunk, c - c0);
            float acc[kMergeChunk];
#pragma unroll
            for (int k = 0; k < kMergeChunk; ++k) acc[k] = 0.0f;
            cnt = 0;
            for (int j = lb; j < le; ++j) {
                const int i = tile_items[j];
                if ((unsigned)i >= (unsigned)n) continue;
                const int* r = rects + (size_t)i * 4;
                const bool in = X >= r[0] && X < r[2] && Y >= r[1] && Y < r[3];
                const float* v = values + (size_t)i * c + c0;
#pragma unroll
                for (int k = 0; k < kMergeChunk; ++k) {
                    if (k < cc) {
                        const float s = acc[k] + v[k];
                        acc[k] = in ? s : acc[k];
                    }
                }
                cnt += in ? 1 : 0;
            }
            const double den = (double)cnt + 1e-8;
#pragma unroll
            for (int k = 0; k < kMergeChunk; ++k) {
                if (k < cc) {
                    if (sum) sum[pix * c + c0 + k] = acc[k];
                    if (raw) raw[pix * c + c0 + k] = (float)((double)acc[k] / den);
                    if ((c0 == 0 && k == 0) || acc[k] > bestv) {
                        bestv = acc[k];
                        best = c0 + k;
                    }
                }
            }
        }
        if (count) count[pix] = cnt;
        if (labels) labels[pix] = (L)(cnt > 0 ? best + 1 : 0);
    }
}


// ---- merge_attention: per-patch attention grids resampled into a whole-slide map ------------------------------------------
// The arithmetic is stated once, in models/engine/_attention_merge.py.  Patch i brings a grid maps[i, k, :, :] of gh x gw cells
// instead of one row of values; a covered pixel (Y, X) samples it at gx = ax * float(X - X0) + cx, gy = ay * float(Y - Y0) + cy
// (affine[i] = (ax, cx, ay, cy), made on the host; (X0, Y0) the rectangle's own corner), clamped to the grid, nearest or bilinear,
// every float32 operation rounded on its own, so that NumPy float32 gives the same bits: plain operators under this file's
// `#pragma clang fp contract(off)`.  (NOT __fmul_rn / __fadd_rn: in this toolchain's headers they are `x * y` / `x + y` compiled under the
// headers' default contraction, and once inlined a __fadd_rn(__fmul_rn(..), ..) becomes one fma -- seen on the device as 295 differing
// sums on a 64 x 48 map.)  The structure is merge_patch_rects_kernel's: a workgroup owns a tile and walks its ascending list;
// the item, its rectangle and its affine are wave-uniform; a pixel computes its cell indices and weights once per patch and
// uses them for up to kMergeChunk channels held in registers (further channels: further passes, order unchanged).  The clamp
// keeps every index inside the grid whatever the affine holds (NaN included: fmaxf / fminf return the other operand; gw - 1 and
// gh - 1 are exact in float32 because the entry point refuses a grid side above 2^24), so the gathers cannot leave `maps`; a
// patch's grid is a few KB at most and stays in cache.  With neither `sum` nor `raw` wanted the walk only counts: one pass, no
// gathers.  Outputs are planar ([c, h, w]): consecutive lanes take consecutive X and store consecutive floats.  No atomics.
template <int MODE>
__global__ __launch_bounds__(CT) void merge_patch_grids_kernel(const int* __restrict__ rects, const float* __restrict__ affine,
                                                                const float* __restrict__ maps, int n, int c, int gh, int gw, int h, int w,
                                                                const int* __restrict__ tile_offsets, const int* __restrict__ tile_items,
                                                                int tile_h, int tile_w, int tiles_x, float* __restrict__ sum,
                                                                float* __restrict__ raw, int* __restrict__ count) {
    const int tile = (int)blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * tile_h, x0 = tx * tile_w;
    const int th = min(tile_h, h - y0), tw = min(tile_w, w - x0);
    const int lb = tile_offsets[tile], le = tile_offsets[tile + 1];
    const size_t cells = (size_t)gh * gw, plane = (size_t)h * w;
    const float xmax = (float)(gw - 1), ymax = (float)(gh - 1);
    const bool sample = sum != nullptr || raw != nullptr;
    const int c_end = sample ? c : 1;  // (coverage alone: one walk of the list)
    for (int p = threadIdx.x; p < th * tw; p += CT) {
        const int py = p / tw;
        const int X = x0 + (p - py * tw), Y = y0 + py;
        const size_t pix = (size_t)Y * w + X;
        int cnt = 0;
        for (int c0 = 0; c0 < c_end; c0 += kMergeChunk) {
            const int cc = min(kMergeChunk, c - c0);
            float acc[kMergeChunk];
#pragma unroll
            for (int k = 0; k < kMergeChunk; ++k) acc[k] = 0.0f;
            cnt = 0;
            for (int j = lb; j < le; ++j) {
                const int i = tile_items[j];
                if ((unsigned)i >= (unsigned)n) continue;
                const int* r = rects + (size_t)i * 4;
                const int rx0 = r[0], ry0 = r[1];
                if (!(X >= rx0 && X < r[2] && Y >= ry0 && Y < r[3])) continue;
                ++cnt;
                if (!sample) continue;
                const float* a = affine + (size_t)i * 4;
                float gx = a[0] * (float)(X - rx0) + a[1];  // (two roundings: see above)
                float gy = a[2] * (float)(Y - ry0) + a[3];
                gx = fminf(fmaxf(gx, 0.0f), xmax);
                gy = fminf(fmaxf(gy, 0.0f), ymax);
                const float* g = maps + ((size_t)i * c + c0) * cells;
                if (MODE == 0) {
                    const int jx = min((int)floorf(gx + 0.5f), gw - 1), jy = min((int)floorf(gy + 0.5f), gh - 1);
                    const size_t o = (size_t)jy * gw + jx;
#pragma unroll
                    for (int k = 0; k < kMergeChunk; ++k) {
                        if (k < cc) acc[k] = acc[k] + g[o];
                        g += cells;  // (a running pointer: sixteen hoisted 64-bit channel offsets would not fit the scalar registers)
                    }
                } else {
                    const int jx0 = (int)floorf(gx), jy0 = (int)floorf(gy);
                    const float wx = gx - (float)jx0, wy = gy - (float)jy0;
                    const int jx1 = min(jx0 + 1, gw - 1), jy1 = min(jy0 + 1, gh - 1);
                    const size_t o00 = (size_t)jy0 * gw + jx0, o01 = (size_t)jy0 * gw + jx1;
                    const size_t o10 = (size_t)jy1 * gw + jx0, o11 = (size_t)jy1 * gw + jx1;
#pragma unroll
                    for (int k = 0; k < kMergeChunk; ++k) {
                        if (k < cc) {
                            const float v00 = g[o00], v01 = g[o01], v10 = g[o10], v11 = g[o11];
                            const float top = v00 + wx * (v01 - v00);
                            const float bot = v10 + wx * (v11 - v10);
                            acc[k] = acc[k] + (top + wy * (bot - top));
                        }
                        g += cells;
                    }
                }
            }
            const double den = (double)cnt + 1e-8;
            size_t o = (size_t)c0 * plane + pix;
#pragma unroll
            for (int k = 0; k < kMergeChunk; ++k) {
                if (k < cc) {
                    if (sum) sum[o] = acc[k];
                    if (raw) raw[o] = (float)((double)acc[k] / den);
                }
                o += plane;
            }
        }
        if (count) count[pix] = cnt;
    }
}


// ---- patch reads from an in-memory slide level ---------------------------------------------------------------------
// WSIPatchDataset.__getitem__ / read_bounds(..., pad_constant_values=255) (models/dataset/dataset_abc.py:418-448) for a
// whole batch of equally sized bounds at once: out[m, y, x, :] = slide[y0+y, x0+x, :] or `pad` outside the slide.
// One thread produces 4 consecutive output bytes (one dword store; rows of ph*pw*c bytes are dword multiples, checked
// by the launcher), reading the source with one dword load when the source run is in bounds and aligned.
__global__ __launch_bounds__(CT) void gather_patches_kernel(const uint8_t* __restrict__ slide, int sh, int sw, int c,
                                                             const int* __restrict__ bounds, int ph, int pw, int pad,
                                                             uint8_t* __restrict__ out) {
    const long row_bytes = (long)pw * c;
    const long patch_bytes = (long)ph * row_bytes;
    const int m = blockIdx.y;
    const int x0 = bounds[m * 4 + 0], y0 = bounds[m * 4 + 1];
    uint8_t* dst = out + (size_t)m * patch_bytes;
    const uint32_t pad4 = 0x01010101u * (uint32_t)(pad & 255);
    for (long i = ((long)blockIdx.x * CT + threadIdx.x) * 4; i < patch_bytes; i += (long)gridDim.x * CT * 4) {
        const int y = (int)(i / row_bytes);
        const long xb = i - (long)y * row_bytes;       // byte offset inside the patch row
        const int sy = y0 + y;
        uint32_t v = pad4;
        if (sy >= 0 && sy < sh) {
            const long sb = (long)x0 * c + xb;         // byte offset inside the slide row (may be negative)
            const uint8_t* srow = slide + (size_t)sy * sw * c;
            const long lim = (long)sw * c;
            if (sb >= 0 && sb + 4 <= lim && xb + 4 <= row_bytes) {
                const uint8_t* sp = srow + sb;
                if ((reinterpret_cast<uintptr_t>(sp) & 3) == 0) {
                    v = *reinterpret_cast<const uint32_t*>(sp);
                } else {
                    v = (uint32_t)sp[0] | ((uint32_t)sp[1] << 8) | ((uint32_t)sp[2] << 16) | ((uint32_t)sp[3] << 24);
                }
            } else {  // the dword straddles the slide edge or the end of the patch row: byte by byte
                v = 0;
                for (int k = 0; k < 4; ++k) {
                    long xk = xb + k;
                    int yk = y;
                    if (xk >= row_bytes) {  // next patch row
                        xk -= row_bytes;
                        ++yk;
                    }
                    const int syk = y0 + yk;
                    const long sbk = (long)x0 * c + xk;
                    uint32_t b = (uint32_t)(pad & 255);
                    if (yk < ph && syk >= 0 && syk < sh && sbk >= 0 && sbk < lim) b = slide[(size_t)syk * sw * c + sbk];
                    v |= b << (8 * k);
                }
            }
        } else if (xb + 4 > row_bytes) {  // padded row whose dword runs into the next (possibly valid) row
            v = 0;
            for (int k = 0; k < 4; ++k) {
                long xk = xb + k;
                int yk = y;
                if (xk >= row_bytes) {
                    xk -= row_bytes;
                    ++yk;
                }
                const int syk = y0 + yk;
                const long sbk = (long)x0 * c + xk;
                uint32_t b = (uint32_t)(pad & 255);
                if (yk < ph && syk >= 0 && syk < sh && sbk >= 0 && sbk < (long)sw * c) b = slide[(size_t)syk * sw * c + sbk];
                v |= b << (8 * k);
            }
        }
        *reinterpret_cast<uint32_t*>(dst + i) = v;
    }
}


// ---- area-resampled patch reads (a slide read below its baseline resolution) ------------------------------------------
// VirtualWSIReader.read_bounds(..., resolution, units, pad_constant_values=255) (wsicore/wsireader.py): the baseline region,
// padded with `pad` outside the slide, shrunk by an integer factor k with imresize -> cv2.INTER_AREA, i.e. OpenCV's
// resizeAreaFast for uint8 (modules/imgproc/src/resize.cpp): k == 2 is ResizeAreaFastVec, (a + b + c + d + 2) >> 2;
// k >= 3 is saturate_cast<uchar>(float(sum) * (1.0f / (k * k))), rounded half to even.  The box sums stay integers.
// One workgroup owns a tile of tile_h output rows x tile_w output pixels of one patch: the tile's k * tile_h source rows
// are staged in LDS in aligned 16-byte chunks (one dwordx4 load per chunk that lies inside the slide row; only chunks that
// cross the slide edge go byte by byte), then every thread reduces the boxes of 4 consecutive output bytes.  Row r of the
// stage holds the aligned-down source run, so the run's first byte sits at (source address & 15).
constexpr int kAreaStage = 16384;  // LDS bytes of source staged per workgroup (launcher sizes the tile to fit)
constexpr int kAreaUnroll = 4;     // 16-byte chunks each thread has in flight before it writes them to LDS

__device__ __forceinline__ uint32_t area_round(uint32_t sum, int k, float scale) {
    if (k == 1) return sum;
    if (k == 2) return (sum + 2u) >> 2;
    const float v = rintf((float)sum * scale);
    return (uint32_t)(v > 255.0f ? 255.0f : v);
}

// Stages bytes xs .. xs + span - 1 of slide rows sy0 .. sy0 + rows - 1 (either may reach outside the slide; those bytes read as
// `pad`) into LDS rows of nq 16-byte chunks: row r holds the aligned-down run, so its first byte sits at (source address & 15).
// The nt threads of the workgroup share the chunks, kAreaUnroll in flight per thread.
__device__ __forceinline__ void stage_rows(const uint8_t* __restrict__ slide, int sh, long row_bytes, long xs, long sy0, long span,
                                           int rows, int nq, int nt, int pad, uint4* stage4) {
    const int total = rows * nq;
    const uint32_t pad4 = 0x01010101u * (uint32_t)(pad & 255);
    const uintptr_t base = reinterpret_cast<uintptr_t>(slide);
    for (int i0 = threadIdx.x; i0 < total; i0 += nt * kAreaUnroll) {
        uint4 v[kAreaUnroll];
        long lo[kAreaUnroll], sy[kAreaUnroll];
        int need[kAreaUnroll];  // 0: past the window, 1: all pad, 2: one aligned load, 3: byte by byte
#pragma unroll
        for (int u = 0; u < kAreaUnroll; ++u) {
            const int i = i0 + u * nt;
            const int r = i / nq, q = i - r * nq;
            sy[u] = sy0 + r;
            const int a = (int)((base + (uintptr_t)(sy[u] * row_bytes + xs)) & 15);
            lo[u] = xs - a + 16L * q;  // the chunk's byte offset in the slide row; 16-byte aligned in memory
            v[u] = make_uint4(pad4, pad4, pad4, pad4);
            need[u] = 0;
            if (i < total && 16L * q < a + span) {
                need[u] = 1;
                if (sy[u] >= 0 && sy[u] < sh && lo[u] + 16 > 0 && lo[u] < row_bytes)
                    need[u] = (lo[u] >= 0 && lo[u] + 16 <= row_bytes) ? 2 : 3;
            }
            if (need[u] == 2) v[u] = *reinterpret_cast<const uint4*>(slide + sy[u] * row_bytes + lo[u]);
        }
#pragma unroll
        for (int u = 0; u < kAreaUnroll; ++u) {
            if (need[u] == 0) continue;
            if (need[u] == 3) {  // the chunk crosses the left or right edge of the slide
                const uint8_t* rp = slide + sy[u] * row_bytes;
                uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const long o = lo[u] + e;
                    const uint32_t b = (o >= 0 && o < row_bytes) ? (uint32_t)rp[o] : (uint32_t)(pad & 255);
                    w[e >> 2] |= b << (8 * (e & 3));
                }
                v[u] = make_uint4(w[0], w[1], w[2], w[3]);
            }
            stage4[i0 + u * nt] = v[u];  // row i / nq, chunk i % nq: the stage pitch is nq chunks
        }
    }
}

__global__ __launch_bounds__(CT) void gather_area_patches_kernel(const uint8_t* __restrict__ slide, int sh, int sw, int c,
                                                                  const int* __restrict__ bounds, int ph, int pw, int k,
                                                                  int tile_w, int tile_h, int tiles_x, int pitch, int pad,
                                                                  uint8_t* __restrict__ out) {
    extern __shared__ uint4 stage4[];
    uint8_t* stage = reinterpret_cast<uint8_t*>(stage4);
    const int m = blockIdx.y;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int oy0 = ty * tile_h, ox0 = tx * tile_w;
    const int th = min(tile_h, ph - oy0), tw = min(tile_w, pw - ox0);
    const long row_bytes = (long)sw * c;
    const long span = (long)tw * k * c;                          // source bytes of one staged row
    const long xs = ((long)bounds[m * 4 + 0] + (long)ox0 * k) * c;  // the run's byte offset in its slide row (may be < 0)
    const long sy0 = (long)bounds[m * 4 + 1] + (long)oy0 * k;
    const int rows = th * k;
    const uintptr_t base = reinterpret_cast<uintptr_t>(slide);
    stage_rows(slide, sh, row_bytes, xs, sy0, span, rows, pitch >> 4, CT, pad, stage4);
    __syncthreads();
    const int out_row = tw * c;            // output bytes of one tile row
    const int groups = (out_row + 3) >> 2;  // 4-byte groups per tile row
    const float scale = 1.0f / (float)(k * k);
    for (int g = threadIdx.x; g < th * groups; g += CT) {
        const int rr = g / groups, j0 = (g - rr * groups) * 4;
        uint8_t* dst = out + (((size_t)m * ph + oy0 + rr) * pw + ox0) * c;
        uint32_t sums[4] = {0u, 0u, 0u, 0u};
        for (int dy = 0; dy < k; ++dy) {
            const int r = rr * k + dy;
            const int a = (int)((base + (uintptr_t)((sy0 + r) * row_bytes + xs)) & 15);
            const uint8_t* sp = stage + r * pitch + a;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + e;
                if (j >= out_row) break;
                const int ox = j / c, ch = j - ox * c;
                const uint8_t* p = sp + ox * k * c + ch;
                uint32_t s = 0;
                for (int dx = 0; dx < k; ++dx) s += p[dx * c];
                sums[e] += s;
            }
        }
        if (j0 + 4 <= out_row && ((reinterpret_cast<uintptr_t>(dst + j0) & 3) == 0)) {
            *reinterpret_cast<uint32_t*>(dst + j0) = area_round(sums[0], k, scale) | (area_round(sums[1], k, scale) << 8) |
                                                     (area_round(sums[2], k, scale) << 16) | (area_round(sums[3], k, scale) << 24);
        } else {
            for (int e = 0; e < 4 && j0 + e < out_row; ++e) dst[j0 + e] = (uint8_t)area_round(sums[e], k, scale);
        }
    }
}


// ---- area-resampled patch reads at any down-sampling ratio --------------------------------------------------------------
// cv::resize(region, (pw, ph), INTER_AREA) of a wb x hb baseline region for uint8 (modules/imgproc/src/resize.cpp) where
// the two scales are not one integer: computeResizeAreaTab's tap table per axis (double arithmetic, each weight rounded to
// float once) and ResizeArea_Invoker's float accumulation (per source row, the x taps in order into a float; then the
// rows, weighted by the y taps, in order), rint, saturate.  Every product is rounded before its add: the file is compiled
// with fp contract(off).  Unequal integer scales kx != ky take resizeAreaFast's rule instead (kFast): the integer box sum
// times 1.0f / (kx * ky), rinted.  The taps are the same for every patch; each workgroup builds those of its own tile.
// One workgroup owns a tile of tile_h output rows x tile_w output pixels of one patch: it builds the tile's x and y taps in
// LDS, stages the source rows they touch in aligned 16-byte chunks (the staging of gather_area_patches_kernel), then every
// thread computes 4 consecutive output bytes of one output row from LDS and stores them as one dword.
constexpr int kResizeStage = 24576;  // LDS bytes of source staged per workgroup (launcher sizes the tile to fit)

// Taps of destination indices d0 .. d0 + cnt - 1 of an n_src -> n_dst axis: source indices first[i] .. first[i] + num[i] - 1
// (contiguous), weights w[i * max_taps + t].  Fast mode: the k = n_src / n_dst indices of the box, no weights.
__device__ void area_resize_taps(int n_src, int n_dst, int d0, int cnt, int max_taps, bool fast, int* first, int* num, float* w) {
    const double scale = 1.0 / ((double)n_dst / (double)n_src);  // cv::resize: scale_x = 1. / inv_scale_x
    for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
        const int d = d0 + i;
        if (fast) {
            const int k = n_src / n_dst;
            first[i] = d * k;
            num[i] = k;
            continue;
        }
        const double f1 = d * scale, f2 = f1 + scale;
        const double cell = fmin(scale, n_src - f1);
        int s2 = min((int)floor(f2), n_src - 1);
        const int s1 = min((int)ceil(f1), s2);
        float* wd = w + (long)i * max_taps;
        int n = 0;
        const bool left = s1 - f1 > 1e-3;
        if (left) wd[n++] = (float)((s1 - f1) / cell);
        for (int s = s1; s < s2 && n < max_taps; ++s) wd[n++] = (float)(1.0 / cell);
        if (f2 - s2 > 1e-3 && n < max_taps) wd[n++] = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
        first[i] = left ? s1 - 1 : s1;
        num[i] = n;
    }
}

template <bool kFast>
__global__ __launch_bounds__(CT) void gather_area_resize_kernel(const uint8_t* __restrict__ slide, int sh, int sw, int c,
                                                                 const int* __restrict__ bounds, int hb, int wb, int ph, int pw,
                                                                 int tile_w, int tile_h, int tiles_x, int span_cap, int rows_cap,
                                                                 int pitch, int max_taps, int pad, uint8_t* __restrict__ out) {
    extern __shared__ uint4 stage4[];
    uint8_t* stage = reinterpret_cast<uint8_t*>(stage4);
    int* xfirst = reinterpret_cast<int*>(stage + (long)rows_cap * pitch);
    int* xnum = xfirst + tile_w;
    int* yfirst = xnum + tile_w;
    int* ynum = yfirst + tile_h;
    float* xw = reinterpret_cast<float*>(ynum + tile_h);
    float* yw = xw + (long)tile_w * max_taps;
    const int m = blockIdx.y;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int oy0 = ty * tile_h, ox0 = tx * tile_w;
    const int th = min(tile_h, ph - oy0), tw = min(tile_w, pw - ox0);
    area_resize_taps(wb, pw, ox0, tw, max_taps, kFast, xfirst, xnum, xw);
    area_resize_taps(hb, ph, oy0, th, max_taps, kFast, yfirst, ynum, yw);
    __syncthreads();
    // the tile's source window: columns sxa .. sxa + span / c - 1 and rows sya .. sya + rows - 1 of the region (the launcher's
    // caps bound both; the min() only keeps LDS accesses inside the allocation)
    const int sxa = xfirst[0], sya = yfirst[0];
    const long span = (long)min(xfirst[tw - 1] + xnum[tw - 1] - sxa, span_cap) * c;  // source bytes of one staged row
    const int rows = min(yfirst[th - 1] + ynum[th - 1] - sya, rows_cap);
    const long row_bytes = (long)sw * c;
    const long xs = ((long)bounds[m * 4 + 0] + sxa) * c;  // the window's byte offset in its slide row (may be < 0)
    const long sy0 = (long)bounds[m * 4 + 1] + sya;
    const uintptr_t base = reinterpret_cast<uintptr_t>(slide);
    stage_rows(slide, sh, row_bytes, xs, sy0, span, rows, pitch >> 4, CT, pad, stage4);
    __syncthreads();
    const int out_row = tw * c;             // output bytes of one tile row
    const int groups = (out_row + 3) >> 2;  // 4-byte groups per tile row
    const float inv_area = kFast ? 1.0f / (float)((wb / pw) * (hb / ph)) : 0.0f;
    for (int g = threadIdx.x; g < th * groups; g += CT) {
        const int rr = g / groups, j0 = (g - rr * groups) * 4;
        uint8_t* dst = out + (((size_t)m * ph + oy0 + rr) * pw + ox0) * c;
        const int nj = min(4, out_row - j0);
        int off[4], nx[4], px[4];  // per output byte: staged offset of its first x tap, tap count, tile pixel
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = min(j0 + e, out_row - 1);
            px[e] = j / c;
            off[e] = (xfirst[px[e]] - sxa) * c + (j - px[e] * c);
            nx[e] = xnum[px[e]];
        }
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t isum[4] = {0u, 0u, 0u, 0u};
        const int yf = yfirst[rr] - sya, yn = ynum[rr];
        for (int t = 0; t < yn; ++t) {
            const int r = yf + t;
            const int a = (int)((base + (uintptr_t)((sy0 + r) * row_bytes + xs)) & 15);
            const uint8_t* sp = stage + r * pitch + a;
            const float beta = kFast ? 0.0f : yw[rr * max_taps + t];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (e >= nj) break;
                const uint8_t* p = sp + off[e];
                if (kFast) {
                    uint32_t s = 0;
                    for (int u = 0; u < nx[e]; ++u) s += p[u * c];
                    isum[e] += s;
                } else {
                    const float* alpha = xw + px[e] * max_taps;
                    float h = 0.0f;
                    for (int u = 0; u < nx[e]; ++u) h += (float)p[u * c] * alpha[u];
                    const float bh = beta * h;
                    acc[e] = t == 0 ? bh : acc[e] + bh;
                }
            }
        }
        uint32_t b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = rintf(kFast ? (float)isum[e] * inv_area : acc[e]);
            b[e] = (uint32_t)(v > 255.0f ? 255.0f : (v < 0.0f ? 0.0f : v));
        }
        if (nj == 4 && ((reinterpret_cast<uintptr_t>(dst + j0) & 3) == 0)) {
            *reinterpret_cast<uint32_t*>(dst + j0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        } else {
            for (int e = 0; e < nj; ++e) dst[j0 + e] = (uint8_t)b[e];
        }
    }
}


// ---- bicubic patch reads above the slide's resolution -----------------------------------------------------------------
// cv::resize(region, (pw, ph), INTER_CUBIC) of a wb x hb baseline region for uint8 (resize.cpp: resizeGeneric_ with
// HResizeCubic / VResizeCubic and interpolateCubic's A = -0.75): per axis fx = (float)((d + 0.5) * scale - 0.5), s = floor(fx),
// f = fx - s, four float coefficients (no fused multiply-add: the file has fp contract(off)) each rounded half to even to a
// short of 2048 * c; taps s - 1 .. s + 2 clamped to the REGION.  int32 horizontal sums src * alpha per source row, int32
// vertical sums hsum * beta over 4 rows, (v + 2^21) >> 22 saturated.  Every sum is exact, so the order does not matter.
// One workgroup owns a tile of tile_h output rows x tile_w output pixels of one patch: it builds the tile's x and y taps in
// LDS, stages the region rows they touch (stage_rows), then each thread owns 4 consecutive output bytes of the tile row and
// walks down a segment of the tile's rows keeping the horizontal sums of its 4-row source window in registers: each staged
// row is summed once per column, not once per output row that reads it.
constexpr int kCubicStage = 20480;  // LDS bytes of source staged per workgroup (launcher sizes the tile to fit)
constexpr int kCubicRows = 64;      // output rows per tile at most

// Source index s and the four taps' weights (2048 * c, rounded half to even) of output index d at scale = n_src / n_dst.
__device__ __forceinline__ int cubic_taps(int d, double scale, short* w) {
    const float fx = (float)((d + 0.5) * scale - 0.5);
    const int s = (int)floorf(fx);
    const float f = fx - (float)s;
    const float A = -0.75f, x1 = f + 1.0f, g = 1.0f - f;
    float cf[4];
    cf[0] = ((A * x1 - 5.0f * A) * x1 + 8.0f * A) * x1 - 4.0f * A;
    cf[1] = ((A + 2.0f) * f - (A + 3.0f)) * f * f + 1.0f;
    cf[2] = ((A + 2.0f) * g - (A + 3.0f)) * g * g + 1.0f;
    cf[3] = 1.0f - cf[0] - cf[1] - cf[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) w[t] = (short)min(max((int)rintf(cf[t] * 2048.0f), -32768), 32767);
    return s;
}

__global__ __launch_bounds__(CT) void gather_cubic_resize_kernel(const uint8_t* __restrict__ slide, int sh, int sw, int c,
                                                                  const int* __restrict__ bounds, int hb, int wb, int ph, int pw,
                                                                  int tile_w, int tile_h, int tiles_x, int nseg, int span_cap,
                                                                  int rows_cap, int pitch, int pad, uint8_t* __restrict__ out) {
    extern __shared__ uint4 stage4[];
    uint8_t* stage = reinterpret_cast<uint8_t*>(stage4);
    short* xoff = reinterpret_cast<short*>(stage + (long)rows_cap * pitch);  // [tile_w][4] staged byte offset of each x tap
    short* xw = xoff + tile_w * 4;                                           // [tile_w][4] x weights
    short* yw = xw + tile_w * 4;                                             // [tile_h][4] y weights
    int* yq = reinterpret_cast<int*>(yw + tile_h * 4);                       // [tile_h] s - 1 of each output row
    const int m = blockIdx.y;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int oy0 = ty * tile_h, ox0 = tx * tile_w;
    const int th = min(tile_h, ph - oy0), tw = min(tile_w, pw - ox0);
    const double scale_x = 1.0 / ((double)pw / (double)wb), scale_y = 1.0 / ((double)ph / (double)hb);  // as cv::resize
    // the tile's source window: region columns xlo .. xhi and rows ylo .. yhi (taps are monotone in d, clamped to the region;
    // the launcher's caps bound both, the min() only keeps LDS accesses inside the allocation)
    short tmp[4];
    const int xlo = max(cubic_taps(ox0, scale_x, tmp) - 1, 0), xhi = min(cubic_taps(ox0 + tw - 1, scale_x, tmp) + 2, wb - 1);
    const int ylo = max(cubic_taps(oy0, scale_y, tmp) - 1, 0), yhi = min(cubic_taps(oy0 + th - 1, scale_y, tmp) + 2, hb - 1);
    const int cols = min(xhi - xlo + 1, span_cap);
    const int rows = min(yhi - ylo + 1, rows_cap);
    for (int i = threadIdx.x; i < tw + th; i += blockDim.x) {
        if (i < tw) {
            const int s = cubic_taps(ox0 + i, scale_x, xw + i * 4);
#pragma unroll
            for (int t = 0; t < 4; ++t) xoff[i * 4 + t] = (short)((min(max(s - 1 + t, 0), wb - 1) - xlo) * c);
        } else {
            const int r = i - tw;
            yq[r] = cubic_taps(oy0 + r, scale_y, yw + r * 4) - 1;
        }
    }
    const long row_bytes = (long)sw * c;
    const long xs = ((long)bounds[m * 4 + 0] + xlo) * c;  // the window's byte offset in its slide row (may be < 0)
    const long sy0 = (long)bounds[m * 4 + 1] + ylo;
    const uintptr_t base = reinterpret_cast<uintptr_t>(slide);
    stage_rows(slide, sh, row_bytes, xs, sy0, (long)cols * c, rows, pitch >> 4, blockDim.x, pad, stage4);
    __syncthreads();
    const int out_row = tw * c;             // output bytes of one tile row
    const int groups = (out_row + 3) >> 2;  // 4-byte groups per tile row
    const int seg = (int)threadIdx.x / groups;
    if (seg >= nseg) return;
    const int j0 = ((int)threadIdx.x - seg * groups) * 4;
    const int nj = min(4, out_row - j0);
    int off[4][4], alpha[4][4];  // per output byte e and x tap t: staged byte offset, weight
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int j = min(j0 + e, out_row - 1);
        const int px = j / c, ch = j - px * c;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            off[e][t] = xoff[px * 4 + t] + ch;
            alpha[e][t] = xw[px * 4 + t];
        }
    }
    // horizontal sums of region row q (clamped to the region) for the thread's 4 output bytes
    auto hsum = [&](int q, int* h) {
        const int r = min(max(min(max(q, 0), hb - 1) - ylo, 0), rows - 1);
        const int a = (int)((base + (uintptr_t)((sy0 + r) * row_bytes + xs)) & 15);
        const uint8_t* sp = stage + r * pitch + a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int v = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) v += (int)sp[off[e][t]] * alpha[e][t];
            h[e] = v;
        }
    };
    const int rb = seg * th / nseg, re = (seg + 1) * th / nseg;
    int win[4][4];  // horizontal sums of region rows q0 .. q0 + 3 (unclamped indices)
    int q0 = 0;
    for (int rr = rb; rr < re; ++rr) {
        const int q = yq[rr];
        if (rr == rb || q >= q0 + 4) {
#pragma unroll
            for (int t = 0; t < 4; ++t) hsum(q + t, win[t]);
            q0 = q;
        }
        for (; q0 < q; ++q0) {  // slide the window down by one row
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                win[0][e] = win[1][e];
                win[1][e] = win[2][e];
                win[2][e] = win[3][e];
            }
            hsum(q0 + 4, win[3]);
        }
        const short* beta = yw + rr * 4;
        uint32_t b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int v = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) v += win[t][e] * (int)beta[t];
            b[e] = (uint32_t)min(max((v + (1 << 21)) >> 22, 0), 255);
        }
        uint8_t* dst = out + (((size_t)m * ph + oy0 + rr) * pw + ox0) * c + j0;
        if (nj == 4 && ((reinterpret_cast<uintptr_t>(dst) & 3) == 0)) {
            *reinterpret_cast<uint32_t*>(dst) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        } else {
            for (int e = 0; e < nj; ++e) dst[e] = (uint8_t)b[e];
        }
    }
}

}  // namespace tia

using namespace tia;

extern "C" int tia_canvas_row_merge_f32(const float* d_blocks, const int32_t* d_xs, int64_t n, int64_t oh, int64_t ow, int64_t c,
                                         int64_t width, float* d_row, uint8_t* d_cnt, int32_t* d_flags, void* stream) {
    if (!d_blocks || !d_xs || !d_row || !d_cnt || !d_flags) return TIA_EINVAL;
    if (n <= 0 || oh <= 0 || ow <= 0 || c <= 0 || c > 8 || width <= 0 || n > 65535) return TIA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(d_flags, 0, (size_t)n * sizeof(int32_t), st) != hipSuccess) return TIA_ELAUNCH;
    const long per_block = (long)oh * ow * c;
    hipLaunchKernelGGL(block_flags_kernel, dim3(64, (unsigned)n), dim3(CT), 0, st, d_blocks, per_block, d_flags);
    const long total = (long)oh * width;
    long nb = (total + CT - 1) / CT;
    if (nb > 16384) nb = 16384;
    hipLaunchKernelGGL(row_merge_kernel, dim3((unsigned)nb), dim3(CT), 0, st, d_blocks, d_xs, d_flags, (int)n, (int)oh, (int)ow, (int)c,
                       (int)width, d_row, d_cnt);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_canvas_finalize_f32(const float* d_row_a, const uint8_t* d_cnt_a, int64_t ys_a, const float* d_row_b,
                                        const uint8_t* d_cnt_b, int64_t ys_b, int64_t oh, int64_t width, int64_t c, int64_t y_begin,
                                        int64_t y_end, float* d_probs, uint8_t* d_pred, void* stream) {
    if (!d_row_a || !d_cnt_a || !d_pred || (d_row_b && !d_cnt_b)) return TIA_EINVAL;
    if (oh <= 0 || width <= 0 || c <= 0 || c > 255 || y_end < y_begin) return TIA_EINVAL;
    if (y_end == y_begin) return TIA_OK;
    const long total = (y_end - y_begin) * width;
    long nb = (total + CT - 1) / CT;
    if (nb > 16384) nb = 16384;
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)nb), dim3(CT), 0, (hipStream_t)stream, d_row_a, d_cnt_a, (long)ys_a, d_row_b,
                       d_cnt_b, (long)ys_b, (int)oh, (int)width, (int)c, (long)y_begin, (long)y_end, d_probs, d_pred);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_merge_patch_rects_f32(const int32_t* d_rects, const float* d_values, int64_t n, int64_t c, int64_t h, int64_t w,
                                         const int32_t* d_tile_offsets, const int32_t* d_tile_items, int64_t tile_h, int64_t tile_w,
                                         float* d_sum, float* d_raw, int32_t* d_count, void* d_labels, int32_t label_bytes,
                                         void* stream) {
    if (!d_rects || !d_values || !d_tile_offsets || !d_tile_items) return TIA_EINVAL;
    if (!d_sum && !d_raw && !d_count && !d_labels) return TIA_EINVAL;
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || tile_h <= 0 || tile_w <= 0) return TIA_EINVAL;
    if ((label_bytes != 1 && label_bytes != 4) || (label_bytes == 1 && c > 254)) return TIA_EINVAL;
    if (h > 0x7fffffffL || w > 0x7fffffffL || h * w > 0x7fffffffL || n > 0x7fffffffL || c > 0x7fffffffL) return TIA_ESIZE;
    // a tile never reaches past the map (the tile counts do not change): pixels per tile <= h * w < 2^31
    const long th = tile_h < h ? tile_h : h, tw = tile_w < w ? tile_w : w;
    const long tiles_x = (w + tw - 1) / tw, tiles_y = (h + th - 1) / th;
    if (tiles_x * tiles_y * tia::CT > 0xffffffffL) return TIA_ESIZE;  // (a launch holds fewer than 2^32 threads: tiles this small on a map this large)
    hipStream_t st = (hipStream_t)stream;
    if (label_bytes == 1) {
        hipLaunchKernelGGL(tia::merge_patch_rects_kernel<uint8_t>, dim3((unsigned)(tiles_x * tiles_y)), dim3(tia::CT), 0, st, d_rects,
                           d_values, (int)n, (int)c, (int)h, (int)w, d_tile_offsets, d_tile_items, (int)th, (int)tw, (int)tiles_x, d_sum,
                           d_raw, d_count, (uint8_t*)d_labels);
    } else {
        hipLaunchKernelGGL(tia::merge_patch_rects_kernel<int32_t>, dim3((unsigned)(tiles_x * tiles_y)), dim3(tia::CT), 0, st, d_rects,
                           d_values, (int)n, (int)c, (int)h, (int)w, d_tile_offsets, d_tile_items, (int)th, (int)tw, (int)tiles_x, d_sum,
                           d_raw, d_count, (int32_t*)d_labels);
    }
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_merge_patch_grids_f32(const int32_t* d_rects, const float* d_affine, const float* d_maps, int64_t n, int64_t c,
                                         int64_t gh, int64_t gw, int64_t h, int64_t w, const int32_t* d_tile_offsets,
                                         const int32_t* d_tile_items, int64_t tile_h, int64_t tile_w, int32_t mode, float* d_sum,
                                         float* d_raw, int32_t* d_count, void* stream) {
    if (!d_rects || !d_affine || !d_maps || !d_tile_offsets || !d_tile_items) return TIA_EINVAL;
    if (!d_sum && !d_raw && !d_count) return TIA_EINVAL;
    if (n <= 0 || c <= 0 || gh <= 0 || gw <= 0 || h <= 0 || w <= 0 || tile_h <= 0 || tile_w <= 0) return TIA_EINVAL;
    if (mode != 0 && mode != 1) return TIA_EINVAL;
    if (h > 0x7fffffffL || w > 0x7fffffffL || h * w > 0x7fffffffL || n > 0x7fffffffL || c > 0x7fffffffL) return TIA_ESIZE;
    if (gh > (1L << 24) || gw > (1L << 24) || gh * gw > 0x7fffffffL) return TIA_ESIZE;  // (a side above 2^24: gw - 1 is no float32 number)
    const long th = tile_h < h ? tile_h : h, tw = tile_w < w ? tile_w : w;
    const long tiles_x = (w + tw - 1) / tw, tiles_y = (h + th - 1) / th;
    if (tiles_x * tiles_y >= (1L << 24)) return TIA_ESIZE;
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0) {
        hipLaunchKernelGGL(tia::merge_patch_grids_kernel<0>, dim3((unsigned)(tiles_x * tiles_y)), dim3(tia::CT), 0, st, d_rects, d_affine,
                           d_maps, (int)n, (int)c, (int)gh, (int)gw, (int)h, (int)w, d_tile_offsets, d_tile_items, (int)th, (int)tw,
                           (int)tiles_x, d_sum, d_raw, d_count);
    } else {
        hipLaunchKernelGGL(tia::merge_patch_grids_kernel<1>, dim3((unsigned)(tiles_x * tiles_y)), dim3(tia::CT), 0, st, d_rects, d_affine,
                           d_maps, (int)n, (int)c, (int)gh, (int)gw, (int)h, (int)w, d_tile_offsets, d_tile_items, (int)th, (int)tw,
                           (int)tiles_x, d_sum, d_raw, d_count);
    }
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_gather_patches_u8(const uint8_t* d_slide, int64_t sh, int64_t sw, int64_t c, const int32_t* d_bounds,
                                     int64_t m, int64_t ph, int64_t pw, int32_t pad, uint8_t* d_out, void* stream) {
    if (!d_slide || !d_bounds || !d_out || sh <= 0 || sw <= 0 || c <= 0 || m < 0 || ph <= 0 || pw <= 0) return TIA_EINVAL;
    if (m == 0) return TIA_OK;
    const long patch_bytes = (long)ph * pw * c;
    if ((patch_bytes & 3) != 0 || m > 65535 || sh > 0x7fffffffL || sw * c > 0x7fffffffL) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_out) & 3) != 0) return TIA_EINVAL;
    long blocks = (patch_bytes / 4 + tia::CT - 1) / tia::CT;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(tia::gather_patches_kernel, dim3((unsigned)blocks, (unsigned)m), dim3(tia::CT), 0, (hipStream_t)stream,
                       d_slide, (int)sh, (int)sw, (int)c, d_bounds, (int)ph, (int)pw, pad, d_out);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_gather_area_patches_u8(const uint8_t* d_slide, int64_t sh, int64_t sw, int64_t c, const int32_t* d_bounds,
                                          int64_t m, int64_t ph, int64_t pw, int64_t factor, int32_t pad, uint8_t* d_out,
                                          void* stream) {
    if (!d_slide || !d_bounds || !d_out || sh <= 0 || sw <= 0 || (c != 1 && c != 3) || m < 0 || ph <= 0 || pw <= 0 || factor < 1)
        return TIA_EINVAL;
    if (m == 0) return TIA_OK;
    if (factor > 64 || sh > 0x7fffffffL || sw * c > 0x7fffffffL || ph * factor > 0x7fffffffL || pw * factor * c > 0x7fffffffL)
        return TIA_ESIZE;
    // tile: as many output pixels per row as fit k staged rows in kAreaStage bytes, then as many output rows as fit
    const long k = factor;
    long tile_w = (tia::kAreaStage / k - 32) / (k * c);
    tile_w = tile_w < 1 ? 1 : (tile_w > pw ? pw : tile_w);
    const long pitch = ((tile_w * k * c + 15) & ~15L) + 16;  // the run plus up to 15 bytes of alignment in front
    long tile_h = tia::kAreaStage / (k * pitch);
    tile_h = tile_h < 1 ? 1 : (tile_h > ph ? ph : tile_h);
    const long tiles_x = (pw + tile_w - 1) / tile_w, tiles_y = (ph + tile_h - 1) / tile_h;
    if (tiles_x * tiles_y > 0x7fffffffL) return TIA_ESIZE;
    const size_t lds = (size_t)(tile_h * k * pitch);
    const long patch_bytes = ph * pw * c;
    for (long s = 0; s < m; s += 65535) {
        const long n = m - s < 65535 ? m - s : 65535;
        hipLaunchKernelGGL(tia::gather_area_patches_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(tia::CT), lds,
                           (hipStream_t)stream, d_slide, (int)sh, (int)sw, (int)c, d_bounds + s * 4, (int)ph, (int)pw, (int)k,
                           (int)tile_w, (int)tile_h, (int)tiles_x, (int)pitch, pad, d_out + s * patch_bytes);
        if (hipGetLastError() != hipSuccess) return TIA_ELAUNCH;
    }
    return TIA_OK;
}

extern "C" int tia_gather_area_resize_u8(const uint8_t* d_slide, int64_t sh, int64_t sw, int64_t c, const int32_t* d_bounds,
                                         int64_t m, int64_t hb, int64_t wb, int64_t ph, int64_t pw, int32_t pad, uint8_t* d_out,
                                         void* stream) {
    if (!d_slide || !d_bounds || !d_out || sh <= 0 || sw <= 0 || (c != 1 && c != 3) || m < 0 || hb <= 0 || wb <= 0 || ph <= 0 ||
        pw <= 0)
        return TIA_EINVAL;
    if (m == 0) return TIA_OK;
    if (sh > 0x7fffffffL || sw * c > 0x7fffffffL || hb > 0x7fffffffL || wb * c > 0x7fffffffL || ph * pw * c > 0x7fffffffL)
        return TIA_ESIZE;
    // cv::resize's scales and its resizeAreaFast test (both scales integers within DBL_EPSILON)
    const double scale_x = 1.0 / ((double)pw / (double)wb), scale_y = 1.0 / ((double)ph / (double)hb);
    if (!(scale_x >= 1.0 && scale_y >= 1.0 && scale_x <= 64.0 && scale_y <= 64.0)) return TIA_ESIZE;
    const long kx = lrint(scale_x), ky = lrint(scale_y);
    const bool fast = fabs(scale_x - (double)kx) < DBL_EPSILON && fabs(scale_y - (double)ky) < DBL_EPSILON;
    if (fast && kx == ky) return tia_gather_area_patches_u8(d_slide, sh, sw, c, d_bounds, m, ph, pw, kx, pad, d_out, stream);
    // tile: the whole output row (at most 1024 bytes, one 4-byte group per thread) unless one tile row's staged source does
    // not fit kResizeStage; then as many output rows as fit.  The caps bound every tile's source window (see the kernel).
    const long max_taps = (long)floor(fmax(scale_x, scale_y)) + 3;
    auto span_cap = [&](long tw) { return (long)floor((double)tw * scale_x) + 4; };
    auto rows_cap = [&](long th) { return (long)floor((double)th * scale_y) + 4; };
    auto pitch_of = [&](long tw) { return ((span_cap(tw) * c + 15) & ~15L) + 16; };  // plus up to 15 bytes of alignment
    long tile_w = pw < 1024 / c ? pw : 1024 / c;
    while (tile_w > 1 && rows_cap(1) * pitch_of(tile_w) > tia::kResizeStage) tile_w = (tile_w + 1) / 2;
    const long tiles_x = (pw + tile_w - 1) / tile_w;
    tile_w = (pw + tiles_x - 1) / tiles_x;
    const long pitch = pitch_of(tile_w);
    long tile_h = (long)((double)(tia::kResizeStage / pitch - 4) / scale_y);
    tile_h = tile_h < 1 ? 1 : (tile_h > ph ? ph : tile_h);
    while (tile_h > 1 && rows_cap(tile_h) * pitch > tia::kResizeStage) --tile_h;
    const long tiles_y = (ph + tile_h - 1) / tile_h;
    tile_h = (ph + tiles_y - 1) / tiles_y;
    if (tiles_x * tiles_y > 0x7fffffffL) return TIA_ESIZE;
    const long rows = rows_cap(tile_h);
    const size_t lds = (size_t)(rows * pitch + (tile_w + tile_h) * (2 + max_taps) * 4);
    if (lds > 65536) return TIA_ESIZE;
    const long patch_bytes = ph * pw * c;
    for (long s = 0; s < m; s += 65535) {
        const long n = m - s < 65535 ? m - s : 65535;
        auto kern = fast ? tia::gather_area_resize_kernel<true> : tia::gather_area_resize_kernel<false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(tia::CT), lds, (hipStream_t)stream, d_slide,
                           (int)sh, (int)sw, (int)c, d_bounds + s * 4, (int)hb, (int)wb, (int)ph, (int)pw, (int)tile_w, (int)tile_h,
                           (int)tiles_x, (int)span_cap(tile_w), (int)rows, (int)pitch, (int)max_taps, pad, d_out + s * patch_bytes);
        if (hipGetLastError() != hipSuccess) return TIA_ELAUNCH;
    }
    return TIA_OK;
}

extern "C" int tia_gather_cubic_resize_u8(const uint8_t* d_slide, int64_t sh, int64_t sw, int64_t c, const int32_t* d_bounds,
                                          int64_t m, int64_t hb, int64_t wb, int64_t ph, int64_t pw, int32_t pad, uint8_t* d_out,
                                          void* stream) {
    if (!d_slide || !d_bounds || !d_out || sh <= 0 || sw <= 0 || (c != 1 && c != 3) || m < 0 || hb <= 0 || wb <= 0 || ph <= 0 ||
        pw <= 0)
        return TIA_EINVAL;
    if (m == 0) return TIA_OK;
    if (sh > 0x7fffffffL || sw * c > 0x7fffffffL || hb > 0x7fffffffL || wb * c > 0x7fffffffL || ph * pw * c > 0x7fffffffL)
        return TIA_ESIZE;
    if (pw < wb || ph < hb) return TIA_ESIZE;  // up-sampling (or the same size) on both axes
    const double scale_x = 1.0 / ((double)pw / (double)wb), scale_y = 1.0 / ((double)ph / (double)hb);
    // tile: the whole output row when it is at most 1024 bytes (one 4-byte group per thread), else column tiles of a multiple
    // of 4 pixels (dword-aligned in the row); as many output rows as fit kCubicStage, at most kCubicRows.  The caps bound every
    // tile's source window: the taps of tw consecutive outputs span at most floor((tw - 1) * scale) + 4 source indices.
    long tile_w = pw;
    if (pw * c > 1024) {
        const long cap = (1024 / c) & ~3L;
        const long tiles = (pw + cap - 1) / cap;
        tile_w = (((pw + tiles - 1) / tiles) + 3) & ~3L;
    }
    const long tiles_x = (pw + tile_w - 1) / tile_w;
    auto span_cap = [&](long tw) { return (long)floor((double)tw * scale_x) + 6; };
    auto rows_cap = [&](long th) { return (long)floor((double)th * scale_y) + 6; };
    const long pitch = ((span_cap(tile_w) * c + 15) & ~15L) + 16;  // plus up to 15 bytes of alignment
    long tile_h = ph < tia::kCubicRows ? ph : tia::kCubicRows;
    while (tile_h > 1 && rows_cap(tile_h) * pitch > tia::kCubicStage) --tile_h;
    const long tiles_y = (ph + tile_h - 1) / tile_h;
    tile_h = (ph + tiles_y - 1) / tiles_y;
    if (tiles_x * tiles_y > 0x7fffffffL) return TIA_ESIZE;
    const long groups = (tile_w * c + 3) / 4;  // 4-byte groups of one tile row: one thread each
    long nseg = tia::CT / groups;              // the tile's rows split into segments when a row needs few threads
    nseg = nseg < 1 ? 1 : (nseg > tile_h ? tile_h : nseg);
    const long threads = ((groups * nseg + 63) / 64) * 64;
    const long rows = rows_cap(tile_h);
    const size_t lds = (size_t)(rows * pitch + tile_w * 16 + tile_h * 12);
    if (threads > tia::CT || lds > 65536) return TIA_ESIZE;
    const long patch_bytes = ph * pw * c;
    for (long s = 0; s < m; s += 65535) {
        const long n = m - s < 65535 ? m - s : 65535;
        hipLaunchKernelGGL(tia::gather_cubic_resize_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3((unsigned)threads),
                           lds, (hipStream_t)stream, d_slide, (int)sh, (int)sw, (int)c, d_bounds + s * 4, (int)hb, (int)wb, (int)ph,
                           (int)pw, (int)tile_w, (int)tile_h, (int)tiles_x, (int)nseg, (int)span_cap(tile_w), (int)rows, (int)pitch,
                           pad, d_out + s * patch_bytes);
        if (hipGetLastError() != hipSuccess) return TIA_ELAUNCH;
    }
    return TIA_OK;
}
