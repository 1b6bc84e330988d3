// Winograd F(4x2, 3x3) form of the 3x3 / stride-1 NHWC convolution in float32 on the gfx950 matrix cores: F(4, 3) over rows x
// F(2, 3) over columns, 24 multiplies per 4 x 2 outputs and (cin, cout) pair -- 3 per output against F(2x2)'s 4 (conv3x3_wino.hip)
// and the direct kernel's 9.  F(4x4) would be 2.25 per output but fails the 1e-5 accuracy gate on the 256- and 512-channel layers
// of resnet18; F(4x2) stays 3 x inside it.
//
//   Y = A4^T [ (G4 g G2^T) . (B4^T d B2) ] A2     per 4 x 2 output tile, 6 x 4 input tile d, 3 x 3 filter g   (Lavin & Gray)
//
//   B4^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]   (points 0, +-1, +-2, inf)
//   G4   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A4^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
//   B2 / G2 / A2: the F(2, 3) matrices of conv3x3_wino.hip.
//
// The kernel is the F(2x2) kernel's structure with the roles of the position grid changed:
// * weights: U = G4 g G2^T in float64, rounded once (tia_conv_pack_weights_wino42_f32), in the same 2 KB blocks as F(2x2) --
//   [pos 24][cin/16][h8 2][cout/64] blocks of [hi 2][64 cout][4 channels] -- so a weight stage (8 channels) is 24 x 2 KB = 48 KB.
// * a 512-thread workgroup owns 32 tiles (16 x 16 output pixels of one image, or four images of <= 8 x 8) x 64 output channels x
//   all 24 positions; 8 waves = 4 position COLUMNS j x 2 row halves h (positions (3 h + 0..2, j)); every wave holds all 32 tiles, so
//   the 32 x 32 x 2 MFMA and its lane layout are the F(2x2) kernel's: 3 positions x 2 channel tiles x 16 = 96 accumulators.
// * per step (8 input channels) a lane reads 5 patch rows x 2 columns of its tile (rows 0..4 for h = 0, 1..5 for h = 1: the rows
//   its three F(4, 3) outputs use), forms the column combine of its j (d[c] +- d[c']) and three rows of B4^T over them, reads 6
//   weight units and issues 24 MFMAs: 38 vector / LDS instructions beside 24 MFMAs (F(2x2): 32 beside 32), 25 % fewer MFMAs per
//   output.  The column combine is formed by both row halves (10 packed adds); the rows of B4^T are split between them.
// * LDS patch images: the F(2x2) kernel's pair layout (tiles two pixels apart along a row: units {0, 9, 2, 11} + 4 k), with row
//   pitches chosen for tiles FOUR rows apart -- W16: ROW = 82 (4 ROW = 8 mod 16: tile rows shift by {0, 8, 0, 8}), W8: ROW = 48
//   (4 ROW = 0 mod 16) and image pitch 484 (= 4 mod 16: the four images shift by {0, 4, 8, 12}) -- so the 16 lanes of every service
//   group of a ds_read_b128 hit 16 different bank groups, as in conv3x3_wino.hip.
// * epilogue: every wave holds the same (tile, channel) lane layout, so the output transform is lane to lane: the rows of A4^T over
//   the wave's own three positions in registers, the two row halves summed through a 64 KB exchange area in two rounds (a = 0, 1 into
//   h = 0, then a = 2, 3 into h = 1), the column transform (A2, over the four waves j) as in F(2x2), then the float32 tile, bias,
//   residual, ReLU and 16-byte stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tiatoolbox_amd.h"
#include "conv3x3_wino.hpp"
#include "dev_env.hpp"

namespace {

using namespace tia;

struct Wino42Dims {
    int n, h, w, cin, cout, ho, wo, pad_y, pad_x;
    unsigned x_bytes, u_bytes;
    int pos_stride;  // bytes between consecutive positions of the packed weights: (cin / 16) * (cout / 64) * 4096
};

// a * b + c / -(a * b) + c on a pair, the constant `a` from a scalar register pair
__device__ __forceinline__ f32x2 pk_fma_s(f32x2 a, f32x2 b, f32x2 c) {
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "s"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ f32x2 pk_fnma_s(f32x2 a, f32x2 b, f32x2 c) {
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(r) : "s"(a), "v"(b), "v"(c));
    return r;
}

// LDS patch images (16-byte units; pixel px of a row at (px >> 1) * 9 + (px & 1) * 4, see the bank analysis above)
//   W16: one image, 16 x 16 output pixels = 4 x 8 tiles, patch 18 x 18
//   W8:  four images of at most 8 x 8 = 4 x (2 x 4) tiles, patch 10 x 10 each
struct W16 {
    static constexpr int G = 1, TH = 16, TW = 16, PH = 18, PWD = 18, ROW = 82, IMG = 18 * 82;
};
struct W8 {
    static constexpr int G = 4, TH = 8, TW = 8, PH = 10, PWD = 10, ROW = 48, IMG = 484;
};

// PERSIST: as in conv3x3_wino.hip (one workgroup per CU walks (pixel block, 64-channel tile) items; the next item's first patch slice
// and weight stage are requested by the current item's last slice).  A weight stage of 48 KB makes every persistent map the LATE one:
// [patch 0][stage 0][patch 1][stage 1], the epilogue's 64 KB over patch 1 and the front of stage 1, stage 1's first refill behind it.
template <typename GEO, bool PERSIST>
__global__ __launch_bounds__(512, 2) void conv3x3_wino42_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                                const float* __restrict__ bias, const float* __restrict__ res,
                                                                float* __restrict__ y, Wino42Dims d, int relu, int m_tiles, int tiles_x,
                                                                int tiles_per_image) {
    constexpr int NT = 512, BN = 64;
    constexpr int ROW = GEO::ROW;
    constexpr int BLOCK_PX = 256;                                 // 256 output pixels = 32 tiles
    constexpr int A_UNITS = (GEO::G * GEO::IMG + 63) / 64 * 64;   // patch units (16 bytes), whole waves: 1536 | 1984
    constexpr int NA = (A_UNITS + NT - 1) / NT;                   // DMA pieces per patch: 3 | 4
    constexpr int A_BYTES = A_UNITS * 16;
    constexpr int W_STAGE = 24 * 2048;                            // 24 positions x [8 channels][64 columns] float32
    constexpr int EPI_TILE = BLOCK_PX * BN * 4;
    // one block per workgroup: [patch 0][patch 1][stage 0][stage 1][dump], the epilogue's 64 KB over the front of it
    constexpr int OFF_W = PERSIST ? A_BYTES : 2 * A_BYTES;
    constexpr int OFF_A1 = PERSIST ? A_BYTES + W_STAGE : A_BYTES;
    constexpr int OFF_W1 = PERSIST ? OFF_A1 + A_BYTES : OFF_W + W_STAGE;
    constexpr int OFF_EPI = PERSIST ? OFF_A1 : 0;
    constexpr int MAIN_END = 2 * A_BYTES + 2 * W_STAGE;
    constexpr int DUMP = MAIN_END;  // 1 KB the idle waves of the last patch piece write their zeros to
    static_assert(OFF_EPI + EPI_TILE <= MAIN_END, "the epilogue's area lies inside the main loop's");
    static_assert(DUMP + 1024 <= 160 * 1024, "one workgroup per CU");
    static_assert(NA >= 2 && NA <= 6, "patch pieces are spread over the two steps of a slice");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int bid = blockIdx.x;
    const int xcd_tiles = xcd_share(m_tiles);
    const int n_cs = d.cin >> 4, n_cb = d.cout >> 6;
    int item = 0, item_end = 1, item_step = 1, mt_lo = 0;
    if constexpr (PERSIST) {
        mt_lo = (bid & 7) * xcd_tiles;
        const int mt_hi = mt_lo + xcd_tiles < m_tiles ? mt_lo + xcd_tiles : m_tiles;
        item = bid >> 3, item_step = (int)(gridDim.x >> 3), item_end = (mt_hi - mt_lo) * n_cb;
        if (item >= item_end) return;
    } else {
        if (xcd_tile(bid, m_tiles) >= m_tiles) return;  // every XCD walks a contiguous range of pixel blocks
    }
    int mt_id, cb, img, ty0, tx0;
    auto decode = [&](int it) {
        if constexpr (PERSIST) {
            const int q = it / n_cb;
            mt_id = mt_lo + q, cb = it - q * n_cb;
        } else {
            mt_id = xcd_tile(bid, m_tiles), cb = (int)blockIdx.y;
        }
        img = GEO::G == 1 ? mt_id / tiles_per_image : mt_id * GEO::G;
        const int trem = GEO::G == 1 ? mt_id - img * tiles_per_image : 0;
        ty0 = (trem / tiles_x) * GEO::TH;
        tx0 = (trem - (trem / tiles_x) * tiles_x) * GEO::TW;
    };
    decode(item);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // (vector register: see conv3x3_wino.hip)
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int jcol = wave & 3, hrow = wave >> 2;  // position column j, row half h (positions 3 h .. 3 h + 2); the waves of a SIMD: w, w + 4
    const int pg = hrow;
    const int hi = lane >> 5;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)d.x_bytes, kBufferRsrcFlags);
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(u), 0, (int)d.u_bytes, kBufferRsrcFlags);

    int cen[NA];
    auto make_cen = [&] {
        int tid_l = tid;
        asm volatile("" : "+v"(tid_l));  // (recomputed per item: hoisted out of the item loop, the unit decomposition spills)
#pragma unroll
        for (int r = 0; r < NA; ++r) {
            const int un = NT * r + tid_l;
            const int g = un / GEO::IMG, ug = un - g * GEO::IMG;
            const int py = ug / ROW, rem = ug - py * ROW;
            const int pair = rem / 9, r9 = rem - pair * 9;
            const int px = 2 * pair + (r9 >> 2), chunk = r9 == 8 ? 4 : (r9 & 3);  // (unit 8 of a pair: padding)
            const int iy = ty0 - d.pad_y + py, ix = tx0 - d.pad_x + px;
            const bool inside = g < GEO::G && img + g < d.n && py < GEO::PH && px < GEO::PWD && chunk < 4 && (unsigned)iy < (unsigned)d.h &&
                                (unsigned)ix < (unsigned)d.w;
            cen[r] = inside ? (((img + g) * d.h + iy) * d.w + ix) * d.cin * 4 + 16 * chunk : OOB;
        }
    };
    make_cen();
    // weight staging: a stage = 24 position blocks of 2 KB; DMA round q (0..5) moves positions 4 q + (wave >> 1)
    const int w_voff = (wave_s & 1) * 1024 + lane * 16 + (wave_s >> 1) * d.pos_stride;

    unsigned char* const abuf0 = smem;
    constexpr int A_PITCH = OFF_A1;
    auto wst = [&](int stage) -> unsigned char* { return smem + (stage ? OFF_W1 : OFF_W); };
    auto dma_a = [&](int buf, int r, int cs) {
        unsigned char* dst = (NT * r + wave_s * 64 >= A_UNITS) ? smem + DUMP : abuf0 + buf * A_PITCH + r * (NT * 16) + wave_s * 1024;
        dma16(rx, dst, cen[r], cs * 64);
    };
    auto dma_w = [&](int stage, int s, int cbi) {
#pragma unroll
        for (int q = 0; q < 6; ++q) dma16(ru, wst(stage) + q * 8192 + wave_s * 1024, w_voff, 4 * q * d.pos_stride + (s * n_cb + cbi) * 2048);
    };

    f32x16 acc[3][2];  // [position 3 h + ii of the wave's column][channel tile]
#define TIA_WINO42_CLEAR_ACC()                                            \
    _Pragma("unroll") for (int i_ = 0; i_ < 3; ++i_)                      \
        _Pragma("unroll") for (int ct_ = 0; ct_ < 2; ++ct_)               \
            _Pragma("unroll") for (int e_ = 0; e_ < 16; ++e_) acc[i_][ct_][e_] = 0.0f

    // the lane's tile: MFMA row = lane & 31 = tile t; its 6 x 4 input tile starts at patch pixel (4 ty, 2 tx)
    const int t = lane & 31;
    int fa;
    if constexpr (GEO::G == 1) {
        fa = 4 * (t >> 3) * ROW + (t & 7) * 9 + hi;
    } else {
        fa = (t >> 3) * GEO::IMG + 4 * ((t >> 2) & 1) * ROW + (t & 3) * 9 + hi;
    }
    // weights of the lane: position (3 h + ii, j) = block 4 (3 h + ii) + j of the stage
    const int fb = (12 * hrow + jcol) * 128 + hi * 64 + (lane & 31);

    f32x2 vreg[3][2];     // V of the wave's three positions (step whose MFMAs are next), four channels as two pairs
    u32x4 wq[3][2];       // [ii][channel tile]
    u32x4 pa[5], pb[5];   // raw patch units of the NEXT step: rows h + 0..4, columns ca / cb
    // column combine of position column j (B2): j = 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3
    const int ca = jcol == 0 ? 0 : (jcol == 1 ? 1 : (jcol == 2 ? 2 : 1));
    const int cbc = jcol == 0 ? 2 : (jcol == 1 ? 2 : (jcol == 2 ? 1 : 3));
    const bool plus = jcol == 1;
    const int fa_a = fa + hrow * ROW + px_unit(ca), fa_b = fa + hrow * ROW + px_unit(cbc);
    auto patch_reads = [&](int s) {
        const u32x4* sa = reinterpret_cast<const u32x4*>(abuf0 + ((s >> 1) & 1) * A_PITCH) + 2 * (s & 1);
#pragma unroll
        for (int r = 0; r < 5; ++r) pa[r] = sa[fa_a + r * ROW], pb[r] = sa[fa_b + r * ROW];
    };
    auto weight_reads = [&](int s, int ii) {
        const u32x4* sb = reinterpret_cast<const u32x4*>(wst(s & 1)) + fb;
        wq[ii][0] = sb[ii * 512], wq[ii][1] = sb[ii * 512 + 32];
    };
    auto transform = [&] {
        auto pair_of = [](const u32x4& q, int k) { return f32x2{__uint_as_float(q[2 * k]), __uint_as_float(q[2 * k + 1])}; };
        f32x2 T[5][2];  // column-combined rows h + 0..4
        if (plus) {
#pragma unroll
            for (int r = 0; r < 5; ++r)
#pragma unroll
                for (int k = 0; k < 2; ++k) T[r][k] = pk_add(pair_of(pa[r], k), pair_of(pb[r], k));
        } else {
#pragma unroll
            for (int r = 0; r < 5; ++r)
#pragma unroll
                for (int k = 0; k < 2; ++k) T[r][k] = pk_sub(pair_of(pa[r], k), pair_of(pb[r], k));
        }
        // rows of B4^T over the wave's five rows, two channels per instruction (constants from scalar registers):
        //   h = 0 (rows 0..4): V0 = 4 T0 - 5 T2 + T4, V1 = (T4 - 4 T2) + (T3 - 4 T1), V2 = (T4 - 4 T2) - (T3 - 4 T1)
        //   h = 1 (rows 1..5): V3 = (T3 - T1) + 2 (T2 - T0), V4 = (T3 - T1) - 2 (T2 - T0), V5 = 4 T0 - 5 T2 + T4
        // (12 packed instructions per lane and step; the same arithmetic as 24 scalar v_fma_f32 / v_add_f32, which measured 3 %
        // slower over the 13 layers: what stretches this loop is the number of instructions issued beside the MFMA stream)
        const f32x2 k4 = {4.0f, 4.0f}, k5 = {5.0f, 5.0f}, k2 = {2.0f, 2.0f};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const f32x2 edge = pk_fma_s(k4, T[0][k], pk_fnma_s(k5, T[2][k], T[4][k]));
            if (hrow == 0) {
                const f32x2 a = pk_fnma_s(k4, T[2][k], T[4][k]), b = pk_fnma_s(k4, T[1][k], T[3][k]);
                vreg[0][k] = edge, vreg[1][k] = pk_add(a, b), vreg[2][k] = pk_sub(a, b);
            } else {
                const f32x2 c = pk_sub(T[3][k], T[1][k]), g = pk_sub(T[2][k], T[0][k]);
                vreg[0][k] = pk_fma_s(k2, g, c), vreg[1][k] = pk_fnma_s(k2, g, c), vreg[2][k] = edge;
            }
        }
    };
    auto mfma_i = [&](int ii) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
                acc[ii][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(vreg[ii][k >> 1][k & 1], __uint_as_float(wq[ii][ct][k]), acc[ii][ct], 0, 0, 0);
    };
    auto step_end = [&] {
        wait_vm_lgkm0<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    auto lds_barrier = [] {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    const int n_steps = 2 * n_cs;
#pragma unroll
    for (int r = 0; r < NA; ++r) dma_a(0, r, 0);
    dma_w(0, 0, cb);
    dma_w(1, 1, cb);
    step_end();
    TIA_WINO42_CLEAR_ACC();
    for (bool first_item = true;; first_item = false) {  // (one round unless PERSIST)
    patch_reads(0);
#pragma unroll
    for (int ii = 0; ii < 3; ++ii) weight_reads(0, ii);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    transform();
    // (PERSIST, later items: stage 1's refill, requested behind the epilogue, has to have landed; every wave has left the epilogue's area)
    if (first_item || PERSIST) step_end(); else lds_barrier();
    const int cur_cb = cb, cur_img = img, cur_ty0 = ty0, cur_tx0 = tx0;
    const bool has_next = PERSIST && item + item_step < item_end;
    for (int k = 0; k < n_steps; ++k) {
        const bool next = k + 1 < n_steps;
        auto requests = [&] {
            if (k + 2 < n_steps) {
                dma_w(k & 1, k + 2, cur_cb);
                if ((k & 1) == 0) {
#pragma unroll
                    for (int r = 0; r < NA; ++r) dma_a(((k >> 1) & 1) ^ 1, r, (k >> 1) + 1);
                }
            } else if (PERSIST && has_next) {  // the last slice (n_cs even: buffer 1): the next item's patch and stage 0
                if ((k & 1) == 0) {
                    dma_w(0, 0, cb);
#pragma unroll
                    for (int r = 0; r < NA; ++r) dma_a(0, r, 0);
                }
            }
            if (next) patch_reads(k + 1);
        };
        auto mma = [&](int ii) {
            mfma_i(ii);
            if (next) weight_reads(k + 1, ii);
        };
        if (pg == 1) {
            mma(0);
            requests();
        } else {
            requests();
            mma(0);
        }
        mma(1), mma(2);
        if constexpr (PERSIST) {
            if (has_next && k == n_steps - 3) {
                item += item_step;
                decode(item);
                make_cen();
            }
        }
        if (next) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            transform();
        }
        step_end();
    }

    // ---- output transform ----------------------------------------------------------------------------------------------------
    // rows of A4^T over the wave's three positions M(3 h + ii), per channel tile:
    //   h = 0: P0 = M0 + (M1 + M2), P1 = M1 - M2, P2 = M1 + M2, P3 = M1 - M2
    //   h = 1: P0 = M3 + M4, P1 = 2 (M3 - M4), P2 = 4 (M3 + M4), P3 = 8 (M3 - M4) + M5
    // Q_j(a) = P(h = 0) + P(h = 1) through the exchange area [slot j][q 16][lane 64] float4 (unit q of a lane: z[q >> 3][(q >> 2) & 1]
    // [4 (q & 3) ..]): a = 0, 1 into the h = 0 waves, then a = 2, 3 into the h = 1 waves; then the column transform over j as in F(2x2):
    // Y(a, 0) = (Q0 + Q1) + Q2 by wave j = 0, Y(a, 1) = Q1 + (-Q3 - Q2) by wave j = 3, rows a = 2 h, 2 h + 1.
    f32x16 z[2][2];  // [a - 2 h][channel tile]: this wave's part, then Q_j, then the final rows
    f32x16 sx[2][2];  // what the wave hands to its partner of the other row half
    if (hrow == 0) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            sx[0][ct] = acc[1][ct] + acc[2][ct];  // P2
            sx[1][ct] = acc[1][ct] - acc[2][ct];  // P1 = P3
            z[0][ct] = acc[0][ct] + sx[0][ct];
            z[1][ct] = sx[1][ct];
        }
    } else {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const f32x16 s = acc[0][ct] + acc[1][ct], dd = (acc[0][ct] - acc[1][ct]) * 2.0f;
            sx[0][ct] = s;   // P0
            sx[1][ct] = dd;  // P1
            z[0][ct] = s * 4.0f;                  // P2
            z[1][ct] = dd * 4.0f + acc[2][ct];    // P3
        }
    }
    {
        unsigned xoff = OFF_EPI + lane * 16;
        asm volatile("" : "+v"(xoff));  // one base register + immediate offsets
        float4* const xch = reinterpret_cast<float4*>(smem + xoff);
        constexpr int SLOT = 16 * 64;  // float4 units of one wave's 16 units per lane
        auto put = [&](float4* dst, const f32x16 (&v)[2][2]) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const f32x16& zz = v[q >> 3][(q >> 2) & 1];
                dst[q * 64] = float4{zz[4 * (q & 3)], zz[4 * (q & 3) + 1], zz[4 * (q & 3) + 2], zz[4 * (q & 3) + 3]};
            }
        };
        auto add_from = [&](const float4* src, f32x16 (&v)[2][2]) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float4 p = src[q * 64];
                f32x16& zz = v[q >> 3][(q >> 2) & 1];
                zz[4 * (q & 3)] += p.x, zz[4 * (q & 3) + 1] += p.y, zz[4 * (q & 3) + 2] += p.z, zz[4 * (q & 3) + 3] += p.w;
            }
        };
        // round 1: rows a = 0, 1 into the h = 0 waves; round 2: rows a = 2, 3 into the h = 1 waves
        float4* const own = xch + jcol * SLOT;
        if (hrow == 1) put(own, sx);
        lds_barrier();
        if (hrow == 0) add_from(own, z);
        lds_barrier();
        if (hrow == 0) put(own, sx);
        lds_barrier();
        if (hrow == 1) add_from(own, z);
        lds_barrier();
    }
    // residual and bias of all four chunks of a thread, requested behind the row-half rounds (in front of them the persistent form
    // runs out of registers) and before the column round: one exposed round trip
    constexpr int CHUNKS = BLOCK_PX * BN / 8, ITER = CHUNKS / NT;  // 2048 chunks of 8 columns, 4 per thread
    static_assert(CHUNKS % NT == 0 && NT % (BN / 8) == 0, "whole chunk rounds; a thread keeps its column chunk");
    int tid_e = tid;
    asm volatile("" : "+v"(tid_e));  // (the read-out's pixel decomposition is recomputed per item, not hoisted and spilled)
    const int cc = tid_e % (BN / 8);
    const int col0 = cur_cb * BN + cc * 8;
    float4 b0 = float4{0.0f, 0.0f, 0.0f, 0.0f}, b1 = b0;
    if (bias) {
        b0 = *reinterpret_cast<const float4*>(bias + col0);
        b1 = *reinterpret_cast<const float4*>(bias + col0 + 4);
    }
    int mpix[ITER];
    u32x4 rq[ITER][2];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int row = (tid_e + NT * it) / (BN / 8);
        const int g = row / (GEO::TH * GEO::TW), rg = row - g * (GEO::TH * GEO::TW);
        const int oy = cur_ty0 + rg / GEO::TW, ox = cur_tx0 + rg % GEO::TW;
        const bool live = oy < d.ho && ox < d.wo && cur_img + g < d.n;
        mpix[it] = live ? ((cur_img + g) * d.ho + oy) * d.wo + ox : -1;
        rq[it][0] = rq[it][1] = u32x4{0u, 0u, 0u, 0u};
        if (res && live) {
            const u32x4* rp = reinterpret_cast<const u32x4*>(res + (long)mpix[it] * d.cout + col0);
            rq[it][0] = rp[0];
            rq[it][1] = rp[1];
        }
    }
    {
        unsigned xoff = OFF_EPI + lane * 16;
        asm volatile("" : "+v"(xoff));
        float4* const xch = reinterpret_cast<float4*>(smem + xoff);
        constexpr int SLOT = 16 * 64;
        auto put = [&](float4* dst, const f32x16 (&v)[2][2]) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const f32x16& zz = v[q >> 3][(q >> 2) & 1];
                dst[q * 64] = float4{zz[4 * (q & 3)], zz[4 * (q & 3) + 1], zz[4 * (q & 3) + 2], zz[4 * (q & 3) + 3]};
            }
        };
        // column transform: waves j = 1, 2 park Q1, Q2 in [slot j - 1][h]
        if (jcol == 1 || jcol == 2) put(xch + ((jcol - 1) * 2 + hrow) * SLOT, z);
        lds_barrier();
        auto combine = [&](bool left) {
            const float4* q1 = xch + (0 * 2 + hrow) * SLOT;
            const float4* q2 = xch + (1 * 2 + hrow) * SLOT;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float4 z1 = q1[q * 64], z2 = q2[q * 64];
                f32x16& zz = z[q >> 3][(q >> 2) & 1];
                const float a1[4] = {z1.x, z1.y, z1.z, z1.w}, a2[4] = {z2.x, z2.y, z2.z, z2.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = zz[4 * (q & 3) + k];
                    zz[4 * (q & 3) + k] = left ? (v + a1[k]) + a2[k] : a1[k] + (-v - a2[k]);
                }
            }
        };
        if (jcol == 0) combine(true);
        if (jcol == 3) combine(false);
        lds_barrier();  // every exchange read has returned: the tile may take the area's place
    }
    float* tile = reinterpret_cast<float*>(smem + OFF_EPI);
    // output rows 2 h + ar, column b of this wave's tiles -> the tile.  MFMA result row (e & 3) + 8 (e >> 2) + 4 hi = tile tt; its
    // pixel (4 ty + a, 2 tx + b): a lane part (hi, h, b) plus a compile-time part (e) -- one base register and immediate offsets
    auto to_tile = [&](int b) {
        int lane_px = (GEO::G == 1 ? 8 * hi : 4 * GEO::TW * hi) + 2 * hrow * GEO::TW + b;
        unsigned tbase = OFF_EPI + (lane_px * BN + (lane & 31)) * 4;
        asm volatile("" : "+v"(tbase));
        float* const tl = reinterpret_cast<float*>(smem + tbase);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m0 = (e >> 2) * (GEO::G == 1 ? 4 * GEO::TW : GEO::TH * GEO::TW) + 2 * (e & 3);
#pragma unroll
            for (int ar = 0; ar < 2; ++ar)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) tl[(m0 + ar * GEO::TW) * BN + ct * 32] = z[ar][ct][e];
        }
    };
    if (jcol == 0) to_tile(0);
    if (jcol == 3) to_tile(1);
    lds_barrier();
    {
        const float* t0 = tile;
        float4 o[ITER][2];
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int row = (tid_e + NT * it) / (BN / 8);
            const float4 p0 = *reinterpret_cast<const float4*>(t0 + row * BN + cc * 8), p1 = *reinterpret_cast<const float4*>(t0 + row * BN + cc * 8 + 4);
            float v[8] = {p0.x + b0.x, p0.y + b0.y, p0.z + b0.z, p0.w + b0.w, p1.x + b1.x, p1.y + b1.y, p1.z + b1.z, p1.w + b1.w};
            if (res) {
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
    if (!has_next) break;
    lds_barrier();  // every wave has read the tile: stage 1 may take the next item's second step
    dma_w(1, 1, cb);
    TIA_WINO42_CLEAR_ACC();
    }  // items
#undef TIA_WINO42_CLEAR_ACC
}

// U = G4 g G2^T in float64, rounded once; one thread per (cout, cin) pair
__global__ void wino42_pack_kernel(const float* __restrict__ w_oihw, int cout, int cin, float* __restrict__ packed) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)cout * cin) return;
    const int o = (int)(idx / cin), c = (int)(idx - (long)o * cin);
    double g[3][3], t[6][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) g[r][s] = (double)w_oihw[(idx * 3 + r) * 3 + s];
#pragma unroll
    for (int s = 0; s < 3; ++s) {  // t = G4 g
        t[0][s] = g[0][s] / 4.0;
        t[1][s] = -(g[0][s] + g[1][s] + g[2][s]) / 6.0;
        t[2][s] = -(g[0][s] - g[1][s] + g[2][s]) / 6.0;
        t[3][s] = g[0][s] / 24.0 + g[1][s] / 12.0 + g[2][s] / 6.0;
        t[4][s] = g[0][s] / 24.0 - g[1][s] / 12.0 + g[2][s] / 6.0;
        t[5][s] = g[2][s];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) wino_pack_row(t[i], i, cout, cin, o, c, packed);  // U = t G2^T
}

constexpr int wino42_lds_bytes(int patch_units) { return 2 * (((patch_units + 63) / 64 * 64) * 16) + 2 * 24 * 2048 + 1024; }

int conv3x3_wino42_launch(const float* x, const float* u_packed, const float* bias, const float* residual, float* y, long nb, long h,
                          long w, long cin, long cout, long pad_top, long pad_left, long ho, long wo, int relu, hipStream_t stream) {
    const bool small = ho <= 8 && wo <= 8;
    const long tiles_y = small ? 1 : (ho + 15) / 16, tiles_x = small ? 1 : (wo + 15) / 16;
    const long tiles = small ? (nb + 3) / 4 : nb * tiles_y * tiles_x;
    Wino42Dims d{(int)nb, (int)h, (int)w, (int)cin, (int)cout, (int)ho, (int)wo, (int)pad_top, (int)pad_left,
                 (unsigned)(nb * h * w * cin * 4), (unsigned)(24 * cin * cout * 4), (int)((cin / 16) * (cout / 64) * 4096)};
    const WinoGrid g = wino_grid(true, tiles, cin, cout);
    auto run = [&](auto geo, auto persist) {
        using GEO = decltype(geo);
        constexpr int lds = wino42_lds_bytes(GEO::G * GEO::IMG);
        static_assert(lds <= 160 * 1024, "LDS");
        return launch_dyn_lds<&conv3x3_wino42_kernel<GEO, decltype(persist)::value>>(g.grid, dim3(512), lds, stream, x, u_packed, bias, residual, y,
                                                                                    d, relu, (int)tiles, (int)tiles_x, (int)(tiles_y * tiles_x));
    };
    bool ok;
    if (small && g.persist)
        ok = run(W8{}, std::true_type{});
    else if (small)
        ok = run(W8{}, std::false_type{});
    else if (g.persist)
        ok = run(W16{}, std::true_type{});
    else
        ok = run(W16{}, std::false_type{});
    return ok ? TIA_OK : TIA_ELAUNCH;
}

}  // namespace

namespace tia {

int conv3x3_wino_form(long n, long h, long w, long cin, long cout, long pad) {
    if (n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cout <= 0 || pad < 0 || pad > 2) return TIA_EINVAL;
    if (cin % 16 != 0 || cout % 64 != 0) return TIA_ESIZE;
    static const bool force_f22 = tia::dev_env("TIA_WINO_F22") != nullptr;  // developer switch: F(2x2) everywhere (A/B of the two forms)
    if (force_f22 || pad != 1 || 24L * cin * cout * 4 > 0x7fffffffL) return 0;
    // measured per layer: the 32^2 / 16^2 maps of 256^2 patches (16 x 16 blocks) and maps <= 8 x 8 (four-image blocks)
    // win; the 64^2 map (64 channels, 8 steps per item: the longer epilogue weighs most) is a tie and stays on F(2x2)
    return (h % 16 == 0 && w % 16 == 0 && h <= 32 && w <= 32) || (h <= 8 && w <= 8) ? 1 : 0;
}

}  // namespace tia

extern "C" int tia_conv3x3_wino_form(int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad) {
    return tia::conv3x3_wino_form(n, h, w, cin, cout, pad);
}

extern "C" int tia_conv_pack_weights_wino42_f32(const float* d_w_oihw, int64_t cout, int64_t cin, float* d_packed, void* stream) {
    return tia::wino_pack_run(24, wino42_pack_kernel, d_w_oihw, cout, cin, d_packed, (hipStream_t)stream);
}

extern "C" int tia_conv3x3_wino42_nhwc_f32(const float* d_x, const float* d_u_packed, const float* d_bias, const float* d_residual,
                                           float* d_y, int64_t n, int64_t h, int64_t w, int64_t cin, int64_t cout, int64_t pad_top,
                                           int64_t pad_left, int64_t ho, int64_t wo, int32_t relu, void* stream) {
    return tia::conv3x3_wino_run(24, conv3x3_wino42_launch, d_x, d_u_packed, d_bias, d_residual, d_y, n, h, w, cin, cout, pad_top, pad_left, ho,
                                 wo, relu, (hipStream_t)stream);
}
