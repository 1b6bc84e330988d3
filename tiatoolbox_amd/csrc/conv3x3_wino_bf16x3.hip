// Winograd F(2x2, 3x3) form of the 3x3 / stride-1 NHWC float32 convolution with the 16 per-position GEMMs M = V . U on the gfx950
// BF16 matrix cores, BOTH operands split into three bf16 numbers (the identity is conv_ring_bf16x3.hip's, 4.27):
// float32 in, float32 accumulate.  V = B^T d B is formed in float32 exactly as in conv3x3_wino.hip, U = G g G^T is the float32
// tensor of tia_conv_pack_weights_wino_f32 (float64 transform, one rounding); only the multiplication changes:
//   v u = sum_ij v_i u_j over the parts hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); six of the nine terms carry
//   everything float32 sees and every product is exact in the accumulator of v_mfma_f32_32x32x16_bf16: per 16 channels, 32 x 32
//   tile and position 6 x 32 = 192 matrix cycles instead of 8 x 64 = 512 of v_mfma_f32_32x32x2_f32.
// Per (position, channel tile) the six MFMAs go into ONE accumulator, smallest terms first (V part x U part):
//   lo * hi, hi * lo, mid * mid, mid * hi, hi * mid, hi * hi.
//
// Machinery: conv3x3_wino.hip's 16 x 16 block (W16) -- a 512-thread workgroup owns 64 tiles (16 x 16 output pixels of one image) x
// 64 output channels x 16 positions; 8 waves = 4 position rows i x 2 tile halves, 128 accumulator registers per wave; the raw
// 18 x 18 patch of a 16-channel slice arrives by LDS-DMA in the pair layout (two buffers of 24 KB); persistent item walk with the
// next item's first operands requested behind the current item's last steps; the epilogue (column transform in registers, row
// transform through the exchange area, + bias + residual, ReLU, 16-byte stores) takes the accumulators as they are: the C / D
// layout of v_mfma_f32_32x32x16_bf16 is that of v_mfma_f32_32x32x2_f32.  Any map size is served by these blocks; maps of at
// most 8 x 8 would fill a quarter of one and go FOUR IMAGES to a block instead (W8 below): the same loop and
// epilogue around another decode, patch set-up and tile mapping, those of conv3x3_wino.hip's W8.
//   * a lane's A fragment is row lane & 31 (its tile), k = 8 (lane >> 5) .. + 7: EIGHT channels of the slice, two ds_read_b128 per
//     patch pixel.  Per slice it reads two patch rows x four columns (16 reads), forms R[c] = d[ra] +- d[rb] (32 adds) and keeps
//     the four R in registers; V_j = R0 - R2 | R1 + R2 | R2 - R1 | R1 - R3 (8 adds each, unpacked: a packed float32 add beside the
//     bf16 stream costs more than two plain ones) is split (split_pair: 44 instructions per V_j) right in front of its MFMAs:
//     within a wave the phases follow each other; what overlaps them is the SIMD's other wave (two per SIMD).
//   * weights: three bf16 planes of U in the exact LDS image of a stage.  A whole slice of U (16 positions x 64 columns x 16
//     channels x 3 planes) is 96 KB; a STAGE is (slice, column PAIR jh of the position grid) = 8 positions (i, 2 jh + jl) x
//     [3 planes][2 k-chunks][64 columns][8 bf16] = 48 KB, contiguous in the packed tensor [cin/16][2][cout/64] stages.  A lane's
//     eight k values of a column are one conflict-free ds_read_b128 per (position, plane, channel tile).
//   * a STEP = one stage: step 2 cs + jh does positions j = 2 jh, 2 jh + 1 of slice cs (24 MFMAs per wave).  Top of a step (behind
//     the barrier): request the NEXT step's stage into the other stage buffer (every wave has finished reading it), at jh = 0 also
//     the next slice's patch; end of a step: s_waitcnt vmcnt(0) lgkmcnt(0) and one barrier.
//   * LDS: [patch 0][stage 0][patch 1][stage 1] = 24 + 48 + 24 + 48 = 144 KB; the epilogue's 64 KB lie over patch 1 and the
//     front of stage 1, which the next item requests only behind the epilogue (one barrier); patch 0 and stage 0 hold the next
//     item's first operands while the epilogue runs.  One workgroup per CU, two waves per SIMD, 256 registers.  (W8: patches
//     of 32 KB, 160 KB in all.)
//
// Invalid-input domain: as conv_ring_bf16x3.hip -- a non-finite V, or |V| >= 2^127 (2 - 2^-8), makes every output that reads it
// non-finite, never a finite wrong value; the weights' parts are checked on the host (fused.pack_conv_weights_wino_split).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/tiatoolbox_amd.h"
#include "conv3x3_wino.hpp"
#include "dev_env.hpp"

namespace {

using namespace tia;

struct WinoSplitDims {
    int n, h, w, cin, cout, ho, wo, pad_y, pad_x;
    unsigned x_bytes, u_bytes;
};

// Phase timing (developer builds only: -DTIA_WINO_TIMING=1, build.build(defines=...)): thread 0 of two workgroups prints the
// shader-clock cycles of the prologue, of the steps and of the epilogues, the items it ran, and the sustained shader clock
// (against the constant 100 MHz clock).
#ifndef TIA_WINO_TIMING
#define TIA_WINO_TIMING 0
#endif
#if TIA_WINO_TIMING
#define WSTAMP(var) { const long long now_ = clock64(); var += now_ - tl_; tl_ = now_; }
#else
#define WSTAMP(var)
#endif

// Block geometries: the patch layouts of conv3x3_wino.hip's W16 and W8 (pairs of pixels at 9 units; their bank analysis holds for the
// two units 2 hi, 2 hi + 1 a lane reads here -- the unit offset is the same for all lanes of a service group).
//   W16: 16 x 16 outputs of ONE image, patch 18 x 18, row pitch 84 units: 1536 patch units of 16 bytes, three whole DMA rounds of 512;
//        LDS 24 + 48 + 24 + 48 = 144 KB.  Serves every map size.
//   W8:  FOUR images of at most 8 x 8 outputs, patch 10 x 10 each, row pitch 50 units, image pitch 512 units: 2048 units, four whole
//        DMA rounds; LDS 32 + 48 + 32 + 48 = 160 KB, the whole LDS of a CU.  Block pixel = 64 image + 8 y + x; images beyond
//        the batch and pixels beyond the map read zeros and are never stored.
struct W16 {
    static constexpr int G = 1, TH = 16, TW = 16, PH = 18, PWD = 18, ROW = 84, IMG = 18 * 84;
};
struct W8 {
    static constexpr int G = 4, TH = 8, TW = 8, PH = 10, PWD = 10, ROW = 50, IMG = 512;
};
constexpr int W_STAGE = 8 * 3 * 2048;          // 8 positions x 3 planes x [2 k-chunks][64 columns][8 bf16]
template <typename GEO>
constexpr int wino_split_lds_bytes() {
    return 2 * ((GEO::G * GEO::IMG + 63) / 64 * 64) * 16 + 2 * W_STAGE;
}

template <typename GEO, bool PERSIST>
__global__ __launch_bounds__(512, 2) void conv3x3_wino_bf16x3_kernel(const float* __restrict__ x, const void* __restrict__ u,
                                                                     const float* __restrict__ bias, const float* __restrict__ res,
                                                                     float* __restrict__ y, WinoSplitDims d, int relu, int m_tiles,
                                                                     int tiles_x, int tiles_per_image) {
    constexpr int NT = 512, BN = 64, BLOCK_PX = 256;
    constexpr int TH = GEO::TH, TW = GEO::TW, PH = GEO::PH, PWD = GEO::PWD, ROW = GEO::ROW;
    constexpr int A_UNITS = (GEO::G * GEO::IMG + 63) / 64 * 64, A_BYTES = A_UNITS * 16, LDS_BYTES = wino_split_lds_bytes<GEO>();
    constexpr int NA = A_UNITS / NT;
    constexpr int NW = W_STAGE / (NT * 16);        // DMA rounds per stage: 6
    constexpr int OFF_W = A_BYTES, OFF_A1 = A_BYTES + W_STAGE, OFF_W1 = OFF_A1 + A_BYTES, OFF_EPI = OFF_A1;
    constexpr int EPI_BYTES = BLOCK_PX * BN * 4;
    static_assert(A_UNITS % NT == 0 && W_STAGE % (NT * 16) == 0, "whole DMA rounds: no idle wave, no dump area");
    static_assert(OFF_W1 + W_STAGE == LDS_BYTES && OFF_EPI + EPI_BYTES <= LDS_BYTES && LDS_BYTES <= 160 * 1024, "one workgroup per CU");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#if TIA_WINO_TIMING
    long long tm_pro = 0, tm_steps = 0, tm_epi = 0, tl_ = clock64();
    int n_items_ = 0;
    const long long t0c_ = tl_, t0w_ = wall_clock64();
#endif

    const int bid = blockIdx.x;
    const int xcd_tiles = xcd_share(m_tiles);
    const int n_cs = d.cin >> 4, n_cb = d.cout >> 6;
    // the item walk of conv3x3_wino_kernel: an ITEM = (pixel block mt_id, channel tile cb); PERSIST: workgroup q of XCD x takes items
    // q, q + Q, .. of the XCD's contiguous range of pixel blocks, channel tile fastest
    int item = 0, item_end = 1, item_step = 1, mt_lo = 0;
    if constexpr (PERSIST) {
        mt_lo = (bid & 7) * xcd_tiles;
        const int mt_hi = mt_lo + xcd_tiles < m_tiles ? mt_lo + xcd_tiles : m_tiles;
        item = bid >> 3, item_step = (int)(gridDim.x >> 3), item_end = (mt_hi - mt_lo) * n_cb;
        if (item >= item_end) return;
    } else {
        if (xcd_tile(bid, m_tiles) >= m_tiles) return;
    }
    int mt_id, cb, img, ty0, tx0;
    auto decode = [&](int it) {  // (wave-uniform: scalar registers)
        if constexpr (PERSIST) {
            const int q = it / n_cb;
            mt_id = mt_lo + q, cb = it - q * n_cb;
        } else {
            mt_id = xcd_tile(bid, m_tiles), cb = (int)blockIdx.y;
        }
        img = GEO::G == 1 ? mt_id / tiles_per_image : mt_id * GEO::G;  // (W8: the block's first image; its maps start at (0, 0))
        const int trem = GEO::G == 1 ? mt_id - img * tiles_per_image : 0;
        ty0 = (trem / tiles_x) * TH;
        tx0 = (trem - (trem / tiles_x) * tiles_x) * TW;
    };
    decode(item);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // (a vector register, as in conv3x3_wino_kernel: scalar role branches spill)
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int irow = wave >> 1, wm = wave & 1;  // position row i, tile half
    const int hi = lane >> 5;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)d.x_bytes, kBufferRsrcFlags);
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(u), 0, (int)d.u_bytes, kBufferRsrcFlags);

    // patch staging: unit NT r + tid -> image of the block / row / pixel pair / pixel / unit of the slice (layout above); outside the
    // batch, the image or the patch, and the padding unit of a pair: an out-of-range offset (the DMA writes zeros)
    int cen[NA];
    auto make_cen = [&] {  // for the item `decode` has just set
#pragma unroll
        for (int r = 0; r < NA; ++r) {
            const int un = NT * r + tid;
            const int g = GEO::G == 1 ? 0 : un / GEO::IMG, ug = un - g * GEO::IMG;  // (A_UNITS = G IMG for W8: g < G)
            const int py = ug / ROW, rem = ug - py * ROW;
            const int pair = rem / 9, r9 = rem - pair * 9;
            const int px = 2 * pair + (r9 >> 2), chunk = r9 == 8 ? 4 : (r9 & 3);
            const int iy = ty0 - d.pad_y + py, ix = tx0 - d.pad_x + px;
            const bool inside = img + g < d.n && py < PH && px < PWD && chunk < 4 && (unsigned)iy < (unsigned)d.h && (unsigned)ix < (unsigned)d.w;
            cen[r] = inside ? (((img + g) * d.h + iy) * d.w + ix) * d.cin * 4 + 16 * chunk : OOB;
        }
    };
    make_cen();
    const int w_voff = wave_s * 1024 + lane * 16;  // a wave's KB of a DMA round of the stage

    auto abuf = [&](int buf) -> unsigned char* { return smem + (buf ? OFF_A1 : 0); };
    auto wst = [&](int stage) -> unsigned char* { return smem + (stage ? OFF_W1 : OFF_W); };
    auto dma_a = [&](int buf, int cs) {
#pragma unroll
        for (int r = 0; r < NA; ++r) dma16(rx, abuf(buf) + r * (NT * 16) + wave_s * 1024, cen[r], cs * 64);
    };
    auto dma_w = [&](int stage, int s, int cbi) {  // stage of step s = 2 cs + jh
#pragma unroll
        for (int q = 0; q < NW; ++q) dma16(ru, wst(stage) + q * (NT * 16) + wave_s * 1024, w_voff, (s * n_cb + cbi) * W_STAGE + q * (NT * 16));
    };

    f32x16 acc[4][2];  // [position j of the wave's row][channel tile]
#define TIA_WINO_CLEAR_ACC()                                              \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                      \
        _Pragma("unroll") for (int ct_ = 0; ct_ < 2; ++ct_)               \
            _Pragma("unroll") for (int e_ = 0; e_ < 16; ++e_) acc[j_][ct_][e_] = 0.0f

    // the lane's tile: MFMA row lane & 31 -> tile 32 wm + (lane & 31), its 4 x 4 input tile starts at patch pixel (2 ty, 2 tx); the
    // lane's k values are channels 8 hi .. 8 hi + 7 = units 2 hi, 2 hi + 1 of a pixel
    const int t = 32 * wm + (lane & 31);
    const int fa = GEO::G == 1 ? 2 * (t >> 3) * ROW + (t & 7) * 9 + 2 * hi
                               : (t >> 4) * GEO::IMG + 2 * ((t >> 2) & 3) * ROW + (t & 3) * 9 + 2 * hi;  // (W8: 16 tiles per image)
    // R = d[ra] +- d[rb]: i = 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3
    const int ra_off = (irow == 0 ? 0 : (irow == 2 ? 2 : 1)) * ROW, rb_off = (irow == 0 || irow == 1 ? 2 : (irow == 2 ? 1 : 3)) * ROW;
    const bool plus = irow == 1;
    const int fa_a = fa + ra_off, fa_b = fa + rb_off;
    // weights of the lane: position block (i, jl) of the stage = 3 planes of [k-chunk 2][column 64] units
    const int fb = irow * 2 * 3 * 128 + hi * 64 + (lane & 31);

    float R[4][8];  // [patch column][channel 8 hi + ..] of the slice in work
    auto load_r = [&](int cs) {
        const u32x4* sa = reinterpret_cast<const u32x4*>(abuf(cs & 1));
#pragma unroll
        for (int q = 0; q < 2; ++q) {  // (one 4-channel unit at a time: 32 registers of raw pixels in flight, not 64)
            u32x4 pa[4], pb[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) pa[c] = sa[fa_a + px_unit(c) + q], pb[c] = sa[fa_b + px_unit(c) + q];
            if (plus) {  // (wave-uniform)
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) R[c][4 * q + e] = add_f32(__uint_as_float(pa[c][e]), __uint_as_float(pb[c][e]));
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int e = 0; e < 4; ++e) R[c][4 * q + e] = sub_f32(__uint_as_float(pa[c][e]), __uint_as_float(pb[c][e]));
            }
        }
    };
    // position j of the wave's row: V_j, its three parts, the six weight fragments, twelve MFMAs (the two channel tiles alternate:
    // each accumulator still sees its six terms in the order above)
    auto position = [&](int j, int stage) {
        // (the reads first: their round trip hides behind the split)
        const u32x4* sb = reinterpret_cast<const u32x4*>(wst(stage)) + fb + (j & 1) * (3 * 128);
        u32x4 bh[2], bm[2], bl[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) bh[ct] = sb[ct * 32], bm[ct] = sb[128 + ct * 32], bl[ct] = sb[256 + ct * 32];
        u32x4 ah, am, al;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // packed register q = channels 8 hi + 2 q, + 1
            float v[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int e = 2 * q + k;
                v[k] = j == 0 ? sub_f32(R[0][e], R[2][e]) : (j == 1 ? add_f32(R[1][e], R[2][e]) : (j == 2 ? sub_f32(R[2][e], R[1][e]) : sub_f32(R[1][e], R[3][e])));
            }
            unsigned ph, pm, pl;
            split_pair(v[0], v[1], ph, pm, pl);
            ah[q] = ph, am[q] = pm, al[q] = pl;
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[j][ct] = mfma_bf16(al, bh[ct], acc[j][ct]);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[j][ct] = mfma_bf16(ah, bl[ct], acc[j][ct]);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[j][ct] = mfma_bf16(am, bm[ct], acc[j][ct]);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[j][ct] = mfma_bf16(am, bh[ct], acc[j][ct]);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[j][ct] = mfma_bf16(ah, bm[ct], acc[j][ct]);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) acc[j][ct] = mfma_bf16(ah, bh[ct], acc[j][ct]);
    };
    auto step_end = [&] {  // every DMA requested so far has landed, every LDS read has returned, in every wave
        wait_vm_lgkm0<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    auto lds_barrier = [] {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // prologue: patch of slice 0 and the stage of step 0
    dma_a(0, 0);
    dma_w(0, 0, cb);
    TIA_WINO_CLEAR_ACC();
    step_end();
    WSTAMP(tm_pro)
    for (;;) {  // items (one round unless PERSIST)
        // PERSIST: the item after this one is decoded at the end of step 2 n_cs - 3 (every patch request of the current item has been
        // issued by then, so its offsets `cen` can be overwritten); the last slice's two steps request its patch and its first stage
        // (n_cs is even: the last slice sits in patch buffer 1)
        const int cur_cb = cb, cur_img = img, cur_ty0 = ty0, cur_tx0 = tx0;
        const bool has_next = PERSIST && item + item_step < item_end;
        for (int cs = 0; cs < n_cs; ++cs) {
            const bool last = cs + 1 == n_cs;
            dma_w(1, 2 * cs + 1, cur_cb);
            if (!last)
                dma_a((cs + 1) & 1, cs + 1);
            else if (has_next)
                dma_a(0, 0);
            load_r(cs);
            position(0, 0);
            position(1, 0);
            step_end();
            if (!last)
                dma_w(0, 2 * cs + 2, cur_cb);
            else if (has_next)
                dma_w(0, 0, cb);
            position(2, 1);
            position(3, 1);
            if constexpr (PERSIST) {
                if (has_next && cs == n_cs - 2) {
                    item += item_step;
                    decode(item);
                    make_cen();
                }
            }
            step_end();
        }
        WSTAMP(tm_steps)

        // ---- output transform (A^T = [1 1 1 0; 0 1 -1 -1]): conv3x3_wino_kernel's epilogue --------------------------------------
        // column transform in registers: Z[b] = M0 + M1 + M2 | M1 - M2 - M3; the row transform Y[0][b] = Z(0) + Z(1) + Z(2),
        // Y[1][b] = Z(1) - Z(2) - Z(3) runs over the four waves of a tile half: waves i = 1, 2 park Z(1), Z(2) in the exchange area,
        // wave i = 0 forms Y[0] = (Z0 + Z1) + Z2 and wave i = 3 Y[1] = Z1 + (-Z3 - Z2), and only those rows go through the float32 tile
        // [BLOCK_PX][64] (it takes the exchange area's place) for the 16-byte read-out
        f32x16 z[2][2];  // [b][channel tile]
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            z[0][ct] = acc[0][ct] + acc[1][ct] + acc[2][ct];
            z[1][ct] = acc[1][ct] - acc[2][ct] - acc[3][ct];
        }
        constexpr int CHUNKS = BLOCK_PX * BN / 8, ITER = CHUNKS / NT;  // 2048 chunks of 8 columns, 4 per thread
        static_assert(CHUNKS % NT == 0 && NT % (BN / 8) == 0, "whole chunk rounds; a thread keeps its column chunk");
        const int cc = tid % (BN / 8);
        const int col0 = cur_cb * BN + cc * 8;
        float4 b0 = float4{0.0f, 0.0f, 0.0f, 0.0f}, b1 = b0;
        if (bias) {
            b0 = *reinterpret_cast<const float4*>(bias + col0);
            b1 = *reinterpret_cast<const float4*>(bias + col0 + 4);
        }
        int mpix[ITER];
        u32x4 rq[ITER][2];
#pragma unroll
        for (int it = 0; it < ITER; ++it) {  // block pixel m = image m / (TH TW) of the block, (ty0 + .. / TW, tx0 + .. % TW)
            const int row = (tid + NT * it) / (BN / 8);
            const int g = GEO::G == 1 ? 0 : row / (TH * TW), rg = row - g * (TH * TW);
            const int oy = cur_ty0 + rg / TW, ox = cur_tx0 + rg % TW;
            const bool live = oy < d.ho && ox < d.wo && cur_img + g < d.n;
            mpix[it] = live ? ((cur_img + g) * d.ho + oy) * d.wo + ox : -1;
            rq[it][0] = rq[it][1] = u32x4{0u, 0u, 0u, 0u};
            if (res && live) {
                const u32x4* rp = reinterpret_cast<const u32x4*>(res + (long)mpix[it] * d.cout + col0);
                rq[it][0] = rp[0];
                rq[it][1] = rp[1];
            }
        }
        float* tile = reinterpret_cast<float*>(smem + OFF_EPI);
        {   // exchange area: [Z(1) | Z(2)][tile half][q 16][lane 64] float4; unit q of a lane = z[q >> 3][(q >> 2) & 1][4 (q & 3) ..]
            unsigned xoff = OFF_EPI + (wm * (16 * 64) + lane) * 16;
            asm volatile("" : "+v"(xoff));  // ONE base register + immediate offsets
            float4* const xch = reinterpret_cast<float4*>(smem + xoff);
            constexpr int SLOT = 2 * 16 * 64;
            if (irow == 1 || irow == 2) {
                float4* dst = xch + (irow - 1) * SLOT;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const f32x16& zz = z[q >> 3][(q >> 2) & 1];
                    dst[q * 64] = float4{zz[4 * (q & 3)], zz[4 * (q & 3) + 1], zz[4 * (q & 3) + 2], zz[4 * (q & 3) + 3]};
                }
            }
            lds_barrier();
            auto combine = [&](bool top) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float4 z1 = xch[q * 64], z2 = xch[SLOT + q * 64];
                    f32x16& zz = z[q >> 3][(q >> 2) & 1];
                    const float a1[4] = {z1.x, z1.y, z1.z, z1.w}, a2[4] = {z2.x, z2.y, z2.z, z2.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float v = zz[4 * (q & 3) + k];
                        zz[4 * (q & 3) + k] = top ? (v + a1[k]) + a2[k] : a1[k] + (-v - a2[k]);
                    }
                }
            };
            if (irow == 0) combine(true);
            if (irow == 3) combine(false);
            lds_barrier();  // every exchange read has returned: the tile may take the area's place
        }
        auto to_tile = [&](int a) {  // output row `a` of this wave's tiles -> the tile
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int tt = 32 * wm + (e & 3) + 8 * (e >> 2) + 4 * hi;  // MFMA result row -> tile
                const int m00 = GEO::G == 1 ? 2 * (tt >> 3) * TW + 2 * (tt & 7) : (tt >> 4) * (TH * TW) + 2 * ((tt >> 2) & 3) * TW + 2 * (tt & 3);
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) tile[(m00 + a * TW + b) * BN + ct * 32 + (lane & 31)] = z[b][ct][e];
            }
        };
        if (irow == 0) to_tile(0);
        if (irow == 3) to_tile(1);
        lds_barrier();
        {
            // every chunk's value is finished (residual consumed) BEFORE the first store (loads and stores share vmcnt)
            float4 o[ITER][2];
#pragma unroll
            for (int it = 0; it < ITER; ++it) {
                const int row = (tid + NT * it) / (BN / 8);
                const float4 p0 = *reinterpret_cast<const float4*>(tile + row * BN + cc * 8), p1 = *reinterpret_cast<const float4*>(tile + row * BN + cc * 8 + 4);
                float v[8] = {p0.x + b0.x, p0.y + b0.y, p0.z + b0.z, p0.w + b0.w, p1.x + b1.x, p1.y + b1.y, p1.z + b1.z, p1.w + b1.w};
                if (res) {  // (dead pixels: zeros, never stored)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        v[k] += __uint_as_float(rq[it][0][k]);
                        v[4 + k] += __uint_as_float(rq[it][1][k]);
                    }
                }
                if (relu) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = v[k] > 0.0f ? v[k] : 0.0f;
                }
                o[it][0] = float4{v[0], v[1], v[2], v[3]};
                o[it][1] = float4{v[4], v[5], v[6], v[7]};
            }
#pragma unroll
            for (int it = 0; it < ITER; ++it) {
                if (mpix[it] >= 0) {
                    float4* yo = reinterpret_cast<float4*>(y + (long)mpix[it] * d.cout + col0);
                    yo[0] = o[it][0];
                    yo[1] = o[it][1];
                }
            }
        }
#if TIA_WINO_TIMING
        ++n_items_;
#endif
        if (!has_next) break;
        lds_barrier();  // every wave has read the tile: step 0 of the next item may request stage 1 and patch 1
        TIA_WINO_CLEAR_ACC();
        WSTAMP(tm_epi)
    }  // items
#undef TIA_WINO_CLEAR_ACC
#if TIA_WINO_TIMING
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    WSTAMP(tm_epi)
    // two workgroups report: an early one and one three quarters through the grid, both on XCD 0
    const int late_ = 8 * (3 * ((int)gridDim.x / 8) / 4);
    if (threadIdx.x == 0 && blockIdx.y == 0 && ((int)blockIdx.x == 0 || (int)blockIdx.x == late_))
        printf("wino split wg %d (cin %d, %d items, %d slices each): prologue %lld  steps %lld  epilogues %lld  | shader clock %.0f MHz\n",
               (int)blockIdx.x, d.cin, n_items_, n_cs, tm_pro, tm_steps, tm_epi,
               100.0 * (double)(clock64() - t0c_) / (double)(wall_clock64() - t0w_));
#endif
}

// parts [3][cout][cin][4][4] float32 (bf16 values: the planes of U[o][c][i][j]) -> [cin/16][2][cout/64] stages of
// [8 positions 2 i + jl][3 planes][2 k-chunks][64 columns][8 bf16]: stage (cs, jh, cb) holds, for position (i, 2 jh + jl), plane p,
// k-chunk q, column col and element e, part p of U[64 cb + col][16 cs + 8 q + e][i][2 jh + jl]
__global__ __launch_bounds__(256) void wino_pack_bf16x3_kernel(const float* __restrict__ parts, int cout, int cin,
                                                               unsigned short* __restrict__ out) {
    const long total = 3L * 16 * cout * cin;
    const int n_cb = cout >> 6;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int e = (int)(idx & 7), col = (int)((idx >> 3) & 63), q = (int)((idx >> 9) & 1);
        long r = idx >> 10;
        const int p = (int)(r % 3);
        r /= 3;
        const int pos8 = (int)(r & 7);
        r >>= 3;
        const int cb = (int)(r % n_cb);
        r /= n_cb;
        const int jh = (int)(r & 1), cs = (int)(r >> 1);
        const int i = pos8 >> 1, j = 2 * jh + (pos8 & 1);
        const long o = 64L * cb + col, ch = 16L * cs + 8 * q + e;
        const float v = parts[((((long)p * cout + o) * cin + ch) * 4 + i) * 4 + j];
        out[idx] = (unsigned short)(__float_as_uint(v) >> 16);  // a bf16 value by contract: the low half is zero
    }
}

// One launch over `nb` images (the signature of conv3x3_wino_launch; `u_packed`: tia_conv_pack_weights_wino_bf16x3)
int conv3x3_wino_bf16x3_launch(const float* x, const float* u_packed, const float* bias, const float* residual, float* y, long nb,
                               long h, long w, long cin, long cout, long pad_top, long pad_left, long ho, long wo, int relu,
                               hipStream_t stream) {
    if (!conv3x3_wino_serves(nb, h, w, cin, cout, pad_top, pad_left, ho, wo) || 96L * cin * cout > 0x7fffffffL) return TIA_ESIZE;
    const WinoSplitDims d{(int)nb, (int)h, (int)w, (int)cin, (int)cout, (int)ho, (int)wo, (int)pad_top, (int)pad_left,
                          (unsigned)(nb * h * w * cin * 4), (unsigned)(96 * cin * cout)};
    auto run = [&](auto geo, long tiles_y, long tiles_x, long tiles) {  // `tiles`: pixel blocks of the launch
        using GEO = decltype(geo);
        constexpr int lds = wino_split_lds_bytes<GEO>();
        static_assert(lds <= 160 * 1024, "one workgroup per CU");
        const WinoGrid g = wino_grid(true, tiles, cin, cout);
        return g.persist ? launch_dyn_lds<&conv3x3_wino_bf16x3_kernel<GEO, true>>(g.grid, dim3(512), lds, stream, x, u_packed, bias, residual, y, d,
                                                                                 relu, (int)tiles, (int)tiles_x, (int)(tiles_y * tiles_x))
                         : launch_dyn_lds<&conv3x3_wino_bf16x3_kernel<GEO, false>>(g.grid, dim3(512), lds, stream, x, u_packed, bias, residual, y, d,
                                                                                  relu, (int)tiles, (int)tiles_x, (int)(tiles_y * tiles_x));
    };
    // Maps of at most 8 x 8 outputs go four images per block (conv3x3_wino_run keeps the groups at whole blocks of four).  That form
    // takes the CU's whole LDS: a device that refuses it is remembered, the refusal is cleared, and the 16 x 16 blocks -- correct for
    // every map size -- serve instead.  Developer switch (TIA_DEV=1): TIA_WINO_SPLIT_NO_W8 forces 16 x 16 blocks (A/B runs, bit identity).
    static const bool no_w8 = tia::dev_env("TIA_WINO_SPLIT_NO_W8") != nullptr;
    static std::atomic<bool> w8_refused{false};
    if (ho <= 8 && wo <= 8 && !no_w8 && !w8_refused.load(std::memory_order_relaxed)) {
        if (run(W8{}, 1, 1, (nb + 3) / 4)) return TIA_OK;
        (void)hipGetLastError();
        w8_refused.store(true, std::memory_order_relaxed);
    }
    const long tiles_y = (ho + 15) / 16, tiles_x = (wo + 15) / 16;
    return run(W16{}, tiles_y, tiles_x, nb * tiles_y * tiles_x) ? TIA_OK : TIA_ELAUNCH;
}

}  // namespace

extern "C" int tia_conv_pack_weights_wino_bf16x3(const float* d_parts, int64_t cout, int64_t cin, void* d_packed, void* stream) {
    if (!d_parts || !d_packed || cout <= 0 || cin <= 0) return TIA_EINVAL;
    if (cin % 16 != 0 || cout % 64 != 0 || 96L * cin * cout > 0x7fffffffL) return TIA_ESIZE;
    hipLaunchKernelGGL(wino_pack_bf16x3_kernel, tia::pack_grid(48L * cout * cin), dim3(256), 0, (hipStream_t)stream, d_parts, (int)cout,
                       (int)cin, static_cast<unsigned short*>(d_packed));
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

extern "C" int tia_conv3x3_wino_bf16x3_nhwc_f32(const float* d_x, const void* d_u_packed3, const float* d_bias, const float* d_residual,
                                                float* d_y, int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad_top,
                                                int64_t pad_left, int64_t ho, int64_t wo, int32_t relu, void* stream) {
    // (24 "positions" of float32 = the 96 cin cout bytes of the three bf16 planes, for the 32-bit offsets into the packed weights)
    return tia::conv3x3_wino_run(24, conv3x3_wino_bf16x3_launch, d_x, static_cast<const float*>(d_u_packed3), d_bias, d_residual, d_y, n, h, w,
                                 cin, cout, pad_top, pad_left, ho, wo, relu, (hipStream_t)stream);
}

// Where conv_algo="auto" takes this form (host only, no device needed).  Three conditions:
//   1. a layer the float32 Winograd forms serve today (tia_conv3x3_wino_form's answer is not negative; "same" padding 1),
//   2. in the persistent form (an even number of 16-channel slices, at least two rounds of items over the compute units: small
//      launches that do not fill the CUs stay where they are), and
//   3. of a layer class that measured faster than the kernel serving it today by more than the spread of three interleaved rounds.
// Measured (scripts/perf_wino.py 4096 256, profiles/wino_split_perf_4096_256.txt; 4096 patches; the float32 form that serves the class
// today -> split, ms; spread of the three rounds in brackets, today's kernel / split):
//     map   channels   serves it today        256^2 patches
//     64^2     64      F(2x2) 16 x 16 blocks   5.62 -> 4.60  x1.22  [0.1 / 0.1 %]
//     32^2    128      F(4x2) 16 x 16 blocks   4.70 -> 3.85  x1.22  [0.0 / 1.0 %]
//     16^2    256      F(4x2) 16 x 16 blocks   4.24 -> 3.50  x1.21  [0.3 / 0.4 %]
//      8^2    512      F(4x2) four images      3.83 -> 11.03 x0.35  [0.2 / 0.1 %]   (a quarter of a 16 x 16 block filled)
// RULE: exactly the three classes measured winning per launch AND in the whole step -- square maps of 64 / 32 / 16
// pixels a side with 64 / 128 / 256 channels in and out.  The maps of 224^2 patches win per launch (4.87 -> 4.34, 4.44 -> 3.74, 4.23 -> 3.40 ms,
// profiles/wino_split_perf_4096_224.txt) but their whole step was not measured with them routed: not admitted yet.  48^2 and rectangular
// maps and other channel counts were not measured; maps of at most 8 x 8 lose on 16 x 16 blocks.
// Four images per block (W8; scripts/perf_wino.py 4096 256 | 224, profiles/wino_split_w8_perf_4096_*.txt):
//     map   channels   serves it today        split, four images per block
//      8^2    512      F(4x2) four images      3.84 -> 3.54  x1.08  [0.2 / 0.6 %]   256^2 patches
//      7^2    512      F(4x2) four images      3.81 -> 3.48  x1.09  [0.1 / 1.2 %]   224^2 patches
// RULE for this geometry, the same as above: the 8^2 / 512 class wins per launch AND in the whole step (71.76 .. 71.93 -> 69.25 .. 69.50 ms,
// DESIGN 4.40 item 4): admitted, answer 2.  The 7^2 / 512 class wins per launch, but the whole step at 224^2 with it routed did not meet
// the criterion (73.94 .. 74.68 -> 73.32 .. 74.11 ms: inside the spread of the runs): NOT admitted.  Other maps of at most 8 x 8 and other
// channel counts were not measured.
// Developer switches (TIA_DEV=1): TIA_WINO_NO_SPLIT makes the answer 0 (A/B runs from one build); TIA_WINO_SPLIT_NO_W8 takes the
// four-image class out (its layers would run on 16 x 16 blocks, which lose).
namespace {

// 0 not taken, 1 one of the three classes on 16 x 16 blocks, 2 the class on four-image blocks; negative: no Winograd form serves it
int wino_split_form(long n, long h, long w, long cin, long cout, long pad) {
    const int form = tia::conv3x3_wino_form(n, h, w, cin, cout, pad);
    if (form < 0) return form;
    static const bool disabled = tia::dev_env("TIA_WINO_NO_SPLIT") != nullptr;
    static const bool no_w8 = tia::dev_env("TIA_WINO_SPLIT_NO_W8") != nullptr;
    if (disabled || pad != 1 || 96L * cin * cout > 0x7fffffffL || h != w || cin != cout) return 0;
    const bool small = h <= 8;  // ("same" padding: the output map is the input's)
    const long tiles = small ? (n + 3) / 4 : n * ((h + 15) / 16) * ((w + 15) / 16);
    if (!tia::wino_grid(true, tiles, cin, cout).persist) return 0;
    if (small) return !no_w8 && h == 8 && cin == 512 ? 2 : 0;
    return (h == 64 && cin == 64) || (h == 32 && cin == 128) || (h == 16 && cin == 256) ? 1 : 0;
}

}  // namespace

extern "C" int tia_conv3x3_wino_bf16x3_form(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad) {
    return wino_split_form(n, h, w, cin, cout, pad);
}

// (the query of DESIGN 4.30: the classes on 16 x 16 blocks only -- 0 for the four-image class)
extern "C" int tia_conv3x3_wino_bf16x3_serves(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad) {
    const int form = wino_split_form(n, h, w, cin, cout, pad);
    return form < 0 ? form : (form == 1 ? 1 : 0);
}
