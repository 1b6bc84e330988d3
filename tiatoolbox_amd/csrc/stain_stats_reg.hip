// Register-resident per-patch statistics kernel (PRODUCT default for Macenko / fixed / given modes, patches of <= 65,536 pixels):
// one 1024-thread workgroup reads the patch from HBM once and keeps it in registers.  DESIGN.md 4.9 / 4.10.
// Reference: tools/stainextract.py:177-227, tools/stainnorm.py:49-66,81-85,103, utils/misc.py:261-290,405-444.
#include "stain_stats_common.hpp"

namespace tia {

// =====================================================================================================================
// Register-resident variant (Macenko / fixed / given modes, patches of <= 65536 pixels with hw % 4 == 0)
// =====================================================================================================================
// ONE 1024-thread workgroup per patch reads the patch from HBM exactly once: thread t keeps the 4-pixel groups
// t, t + 1024, t + 2048, ... (three dwords each, at most 16 of them: 48 VGPRs) for the whole kernel, and every sweep --
// byte histogram, tissue mask + OD moments, the float32 classification sweeps of both selections -- runs out of registers.
// What leaves the registers is small: histogram increments (LDS atomics on a 32-way striped table: lane l owns copy
// l & 31, so the 32 lanes serviced together never share a bank), and the few per cent of pixels that lie inside a selection
// window, appended WITH their colour (r | g << 8 | b << 16 | need-bits << 24) to per-wave LDS lists, so the exact float64
// pass can hand them to any thread.  The statistics are the same numbers, bit for bit, as stain_stats_kernel<false>:
// same table look-ups, same per-pixel instruction sequences -- both kernels call the shared functions of stain_stats_common.hpp
// for them (tables, tissue predicate, moments, eigenvectors, stain vectors, pseudo-inverse, float32 projections) --, the same
// fixed accumulation order (the moments of virtual
// thread t = groups t + 1024 j in ascending order, a wave's shuffle tree, the 16 waves in order -- the streaming kernel
// accumulates in this order too), and exact order statistics.  If a selection window cannot be placed or overflows, the
// patch is flagged in `redo` and the streaming kernel recomputes it (launched right after with the flag array).
constexpr int RT = 1024;
constexpr int RW = RT / 64;
constexpr int RG = 16;        // groups per thread
constexpr int RSEG = 384;     // list entries (16 bytes: one 4-pixel group + need-bits) per wave
constexpr int HCOPY = 32;     // histogram / OD-table copies: lane l uses copy l & 31, so a half-wave never shares a bank
constexpr int L2COPY = 8;     // copies of the float32 log2 table (the sweeps' three transcendental instructions per pixel become look-ups)
constexpr int RCAP = 2048;    // candidates per target (windows over all 65536 pixels of a 256 x 256 patch hold ~800 + slack)

struct SmemR {
    double od[256];
    int ty[3][256];
    unsigned hist[256];
    unsigned cum[256];
    union {  // one 96 KB region, used by one phase at a time
        unsigned hstripe[256 * HCOPY];   // P1: byte histogram, copy (lane & 31) of bin v at v * 32 + (lane & 31)
        double odstripe[256 * HCOPY];    // P2: the float64 OD table, striped the same way (conflict-free look-ups)
        float sbuf[2][SAMPLE_TARGET];    // selections: sample keys (window placement) ...
        uint4 list[RW * RSEG];           // ... then the sweep's lists (the sample is consumed before the sweep starts)
    };
    unsigned sbins[2][SNB];
    double cand[2][RCAP];
    float l2[256 * L2COPY];  // log2(max(v, 1)) of every byte value as the float32 sweeps compute it, copy (lane & 7) of v at v * 8 + copy
    double small[2][64];
    double red[RW][16];
    double tot[16];
    double bc[48];
    int ibc[8];
    WinSel ws;
    unsigned wcnt[RW];
#if TIA_STATS_TIMING
    long long tm[16];
    long long tlast;
#endif
};
#if TIA_STATS_TIMING
#define RSTAMP(i)                                  \
    if (threadIdx.x == 0) {                        \
        const long long now_ = clock64();          \
        s.tm[i] += now_ - s.tlast;                 \
        s.tlast = now_;                            \
    }
#else
#define RSTAMP(i)
#endif

template <int N>
__device__ __forceinline__ void block_sum_r(double (&v)[N], SmemR& s) {
    static_assert(N <= 16, "reduction scratch too small");
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double w = wave_sum(v[i]);
        if (lane_id() == 0) s.red[wave_id()][i] = w;
    }
    __syncthreads();
    // thread i adds the 16 wave partials of value i in wave order (the order block_sum uses), so nobody holds 16 x N values
    if (threadIdx.x < N) {
        double acc = 0.0;
        for (int w = 0; w < RW; ++w) acc += s.red[w][threadIdx.x];
        s.tot[threadIdx.x] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = s.tot[i];
    __syncthreads();
}

// window_select2 for register-resident pixels: this kernel's driver of the shared `wsel_*` stages (stain_stats_common.hpp).
// `sample32(idx, r, g, b, v)` and `exact(r, g, b, x)` as there;
// `sweep(seg, cap, count, below0, below1)` classifies the calling thread's own pixels in float32 and appends the undecided
// ones (colour + need-bits) to this wave's list segment.  Returns false (workgroup-uniform) when a precondition fails.
template <class FETCH, class SAMPLE32, class EXACT, class SWEEP>
__device__ __forceinline__ bool window_select_reg(FETCH&& fetch, long hw, bool shared_keys, SAMPLE32&& sample32,
                                                  EXACT&& exact, SWEEP&& sweep, SmemR& s, const unsigned long long (&k)[2],
                                                  const unsigned long long (&n)[2], double (&vprev)[2], double (&vnext)[2]) {
    const int tid = threadIdx.x;
    WinSel& ws = s.ws;
    if (n[0] == 0 || n[1] == 0) return false;
    constexpr int SPT = SAMPLE_TARGET / RT;  // samples per thread
    unsigned* sbins = &s.sbins[0][0];
    wsel_start<RT>(ws, sbins);
    {
        // the sample comes out of the thread's own registers: thread t holds the groups t + 1024 j -- one every 16 rows of a 256-wide
        // patch, at a column position that runs over the whole row with t -- so one pixel from each quarter of its slots, at a hashed
        // slot and pixel, is a stratified sample over the image (`fetch`).  (Round 3 re-read a strided sample from memory: every
        // sampled byte pulled a whole 64-byte sector, i.e. both selections together re-read ~1.6x the patch: the kernel's HBM-side
        // traffic was 2.8x the patch instead of ~1.2x, profiles/r04s_stain_pmc_*.)
        uint32_t rgb[SPT];
        bool have[SPT];
#pragma unroll
        for (int j = 0; j < SPT; ++j) have[j] = fetch(j, rgb[j]);
        WinSample acc;
        wsel_sample_init(acc);
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            float v[2] = {0.0f, 0.0f};
            const unsigned valid = have[j] ? sample32(0L, rgb[j] & 255u, (rgb[j] >> 8) & 255u, (rgb[j] >> 16) & 255u, v) : 0u;
            wsel_sample_add<RT>(acc, &s.sbuf[0][0], j, valid, v);
        }
        wsel_sample_merge(ws, acc);
    }
    __syncthreads();
    const unsigned ns[2] = {ws.wn[0], ws.wn[1]};
    if (ns[0] < 64u || ns[1] < 64u) return false;
    // (both targets of the angular selection see the same keys: one histogram then serves both)
    wsel_place_windows<RT>(ws, &s.sbuf[0][0], sbins, shared_keys, ns, k, n);
    RSTAMP(TM_SEL_FIND)
    // ---- the float32 sweep over the thread's own pixels ---------------------------------------------------------------------
    {
        unsigned count = 0, bl0 = 0, bl1 = 0;  // count: wave-uniform; bl0 / bl1: per-lane counts of "definitely below"
        sweep(s.list + wave_id() * RSEG, (unsigned)RSEG, count, bl0, bl1);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            bl0 += __shfl_down(bl0, o, 64);
            bl1 += __shfl_down(bl1, o, 64);
        }
        if (lane_id() == 0) {
            s.wcnt[wave_id()] = count;
            if (bl0) atomicAdd(&ws.wbelow[0], (unsigned long long)bl0);
            if (bl1) atomicAdd(&ws.wbelow[1], (unsigned long long)bl1);
        }
    }
    __syncthreads();
    RSTAMP(TM_SEL_HIST)
    {
        bool over = false;
        for (int w = 0; w < RW; ++w) over = over || s.wcnt[w] > (unsigned)RSEG;
        if (over) return false;  // uniform
    }
    // ---- exact classification of the listed pixels: entry e of the concatenated lists goes to thread e % 1024 -----------------
    double* cand = &s.cand[0][0];
    {
        WinExact ex;
        wsel_exact_init(ex);
        unsigned total = 0;
        for (int w = 0; w < RW; ++w) total += s.wcnt[w];
        for (unsigned i = tid; i < total; i += RT) {
            int w = 0;
            unsigned base = 0, acc = 0;
            for (int v = 0; v < RW; ++v) {
                if (i >= acc) {
                    w = v;
                    base = acc;
                }
                acc += s.wcnt[v];
            }
            const uint4 en = s.list[w * RSEG + (i - base)];
            uint32_t rr[4], gg[4], bb[4];
            unpack_group(en.x, en.y, en.z, rr, gg, bb);
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const unsigned need = (en.w >> (2 * px)) & 3u;
                if (!need) continue;
                double x[2];
                exact(rr[px], gg[px], bb[px], x);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (!((need >> t) & 1u)) continue;
                    wsel_exact_add<RCAP>(ws, ex, cand, t, x[t]);
                }
            }
        }
        wsel_exact_merge(ws, ex);
    }
    __syncthreads();
    RSTAMP(TM_SEL_COLLECT)
#if TIA_STATS_TIMING
    if (tid == 0) {
        s.tm[11] += ws.wn[0];
        s.tm[12] += ws.wn[1];
        for (int w = 0; w < RW; ++w) s.tm[13] += s.wcnt[w];
    }
#endif
    if (!wsel_check<RCAP>(ws, k, n)) return false;
    wsel_refine<RT, RCAP>(ws, sbins, cand, &s.small[0][0], &s.bc[40], k, n, vprev, vnext);
    RSTAMP(TM_SEL_SORT)
    return true;
}

// The patch registers are LLVM vectors: a loop over the groups with a (wave-uniform) run-time index then compiles to indexed
// register moves (s_set_gpr_idx / v_movrel) instead of 16 unrolled copies of every sweep -- unrolled, the kernel is > 100 KB of
// straight-line code that every wave streams through the instruction cache once per patch.
using u32x16 = uint32_t __attribute__((ext_vector_type(16)));

// Workgroup-uniform values (read from LDS or computed from such) moved to scalar registers: they are live across the sweeps,
// and the vector registers are needed for the patch.
__device__ __forceinline__ float uni(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }
__device__ __forceinline__ double uni(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Single-lane arithmetic of the register-resident kernel as REAL calls: their (large) register needs then do not add to the
// kernel's own allocation, which is dominated by the 48 registers of the patch; only the calling wave pays the call.  The bodies
// are the shared ones of stain_stats_common.hpp.
__device__ __attribute__((noinline)) void reg_eigen(const double (&acc)[10], double (&cov)[6], double (&e1)[3], double (&e2)[3]) {
    stats_eigen(acc, cov, e1, e2);
}
__device__ __attribute__((noinline)) void reg_stain_from_angles(const double (&vp)[2], const double (&vn)[2], const double (&gm)[2],
                                                                const double (&e1)[3], const double (&e2)[3], double (&phi)[2],
                                                                double (&hv)[3], double (&ev)[3]) {
    stats_stain_from_angles(vp, vn, gm, e1, e2, phi, hv, ev);
}
// log2(max(v, 1)) from the kernel's LDS table (copy `lane & 7`): the float32 sweeps' look-up form of `Log2Insn`
struct Log2Table {
    const float* t;
    __device__ __forceinline__ float operator()(uint32_t v) const { return t[v * L2COPY]; }
};
__device__ __forceinline__ void uni(Proj32<Log2Table>& q) {
    q.a0 = uni(q.a0), q.a1 = uni(q.a1), q.a2 = uni(q.a2), q.ka = uni(q.ka);
    q.b0 = uni(q.b0), q.b1 = uni(q.b1), q.b2 = uni(q.b2), q.kb = uni(q.kb);
}

__global__ __launch_bounds__(RT) void stain_stats_reg_kernel(const uint8_t* __restrict__ img, long hw,
                                                              const tia_stain_tables* __restrict__ tab, tia_stain_params prm,
                                                              double* __restrict__ stats, int* __restrict__ redo,
                                                              uint32_t* __restrict__ sample_ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    SmemR& s = *reinterpret_cast<SmemR*>(smem_raw);
    const uint8_t* p = img + (size_t)blockIdx.x * (size_t)hw * 3u;
    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(p);
    double* out = stats + (size_t)blockIdx.x * TIA_STATS_STRIDE;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool z1 = prm.zero_to_one != 0;
    const int ng = (int)(hw >> 2);

    // ---- the patch: groups tid + 1024 j, all loads in flight together ------------------------------------------------------
    static_assert(RG == 16, "the patch registers are 16-wide vectors");
    u32x16 pa, pb, pc;
#pragma unroll
    for (int j = 0; j < RG; ++j) {
        const int g = tid + RT * j;
        const int gc = g < ng ? g : ng - 1;  // clamped (branch-free loads); slots beyond the patch are never used
        pa[j] = q[gc * 3 + 0];
        pb[j] = q[gc * 3 + 1];
        pc[j] = q[gc * 3 + 2];
    }
    const int n_slots = (ng + RT - 1) / RT;  // group slots in use (workgroup-uniform)
    // The window-placing sample (4 pixels per thread: the stratified sample of sample_index) is requested HERE, right behind the
    // patch itself -- its bytes sit in lines the workgroup's own coalesced loads are bringing into L2 at this moment -- and parked
    // in 16 KB of the patch's (otherwise unused) bin-cache workspace once P1 has run; each selection reads its 4 values back with
    // one coalesced load.  (Round 3 re-read the sample from the image in front of each selection, long after the lines had left
    // L2: every sampled byte pulled a whole 64-byte sector, both selections together re-read ~1.6x the patch and the kernel's
    // HBM-side traffic was 2.8x the patch, profiles/r04s_stain_pmc_*.  Selecting the sample out of the patch registers instead
    // -- a per-lane select chain over the 48 registers -- was measured too: at the point of use it spilled 45 more registers (3.97 ms),
    // at kernel start it made P1 wait for the whole patch and slowed the later sweeps (2.95 ms), profiles/r04t_*, r04u_*.)
    uint32_t* __restrict__ my_samples = sample_ws + (size_t)blockIdx.x * (size_t)hw;  // the patch's own 4 hw bytes of the bin cache
    constexpr int SPT_R = SAMPLE_TARGET / RT;
    uint32_t srgb[SPT_R];
    {
        const long sstride = (hw + SAMPLE_TARGET - 1) / SAMPLE_TARGET;
#pragma unroll
        for (int k = 0; k < SPT_R; ++k) {
            const long idx = sample_index((long)k * RT + tid, sstride);
            const long ic = idx < hw ? idx : hw - 1;
            srgb[k] = ((uint32_t)p[3 * ic] | ((uint32_t)p[3 * ic + 1] << 8) | ((uint32_t)p[3 * ic + 2] << 16)) |
                      (idx < hw ? 0x80000000u : 0u);  // bit 31: a pixel of the patch
        }
    }
    auto fetch_sample = [&](int k, uint32_t& rgb) -> bool {
        const uint32_t v = my_samples[k * RT + tid];
        rgb = v & 0xffffffu;
        return (v >> 31) != 0u;
    };
    double s_given[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (prm.mode == TIA_MODE_GIVEN) {
#pragma unroll
        for (int i = 0; i < 6; ++i) s_given[i] = out[TIA_ST_STAIN + i];
        __syncthreads();
    }
    auto give_up = [&]() {  // workgroup-uniform: hand the patch to the streaming kernel
        if (tid == 0) {
            if (prm.mode == TIA_MODE_GIVEN)
                for (int i = 0; i < 6; ++i) out[TIA_ST_STAIN + i] = s_given[i];
            redo[blockIdx.x] = 1;
        }
    };
#if TIA_STATS_TIMING
    if (tid == 0) {
        for (int i = 0; i < 16; ++i) s.tm[i] = 0;
        s.tlast = clock64();
    }
    const long long t_begin = clock64();
#endif
    if (tid < TIA_STATS_STRIDE) out[tid] = 0.0;
    if (tid < 256) s.od[tid] = tab->od_lut[tid];
    // the SAME instruction the streaming kernel issues per pixel and channel, evaluated once per byte value: identical bits, and
    // the two classification sweeps (12 of their ~58 issue slots per pixel were v_log_f32) read it back from LDS
    for (int i = tid; i < 256 * L2COPY; i += RT) s.l2[i] = Log2Insn{}((uint32_t)(i / L2COPY));
    for (int i = tid; i < 256 * HCOPY; i += RT) s.hstripe[i] = 0u;
    __syncthreads();

    // ---- P1: byte histogram of all three channels together (the percentiles are over the flattened image) ------------------
    {
        unsigned* hs = s.hstripe + (lane & (HCOPY - 1));
#pragma unroll 1
        for (int j = 0; j < n_slots; ++j) {
            if (tid + RT * j < ng) {
                const uint32_t w[3] = {pa[j], pb[j], pc[j]};
#pragma unroll
                for (int d = 0; d < 3; ++d)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        uint32_t v = (w[d] >> (8 * e)) & 255u;
                        if (z1) v = v ? v : 1u;
                        atomicAdd(hs + v * HCOPY, 1u);
                    }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SPT_R; ++k) my_samples[k * RT + tid] = srgb[k];
    RSTAMP(TM_P1)
    if (tid < 256) {
        unsigned tot = 0;
#pragma unroll 8
        for (int c = 0; c < HCOPY; ++c) tot += s.hstripe[tid * HCOPY + ((c + lane) & (HCOPY - 1))];  // rotated: no bank conflicts
        s.hist[tid] = tot;
    }
    __syncthreads();
    {
        double plow, phigh;
        ce_percentiles(s.hist, s.cum, s.ibc, hw, prm.q_img_lo, prm.q_img_hi, plow, phigh);
        if (tid == 0) {
            out[TIA_ST_PLOW] = plow;
            out[TIA_ST_PHIGH] = phigh;
        }
        if (tid < 256) ce_luminance_tables(tab, plow, phigh, z1, tid, s.ty);
    }
    __syncthreads();
    RSTAMP(TM_LUT)
    const int y_thr = prm.y_thr;
    auto sgn = [](float v) -> unsigned { return __float_as_uint(v) >> 31; };  // 1 iff v < 0 (v is never NaN where it counts)

    unsigned flags = 0;
    if (prm.mode == TIA_MODE_MACENKO) {
        // ---- P2: tissue mask (kept as bits in two registers) + OD moments, out of the registers --------------------------------
        for (int i = tid; i < 256 * HCOPY; i += RT) s.odstripe[i] = s.od[i / HCOPY];  // the histogram is consumed: its LDS takes
        __syncthreads();                                                              // the striped OD table
        const double* ods = s.odstripe + (lane & (HCOPY - 1));
        double acc[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) acc[i] = 0.0;
        unsigned long long tmask = 0ull;
#pragma unroll 1
        for (int j = 0; j < n_slots; ++j) {
            const bool valid = tid + RT * j < ng;
            uint32_t rr[4], gg[4], bb[4];
            unpack_group(pa[j], pb[j], pc[j], rr, gg, bb);
            // the luminance look-ups of all four pixels and the OD look-ups of two at a time are in flight together; the
            // accumulation order (pixel 0, 1, 2, 3 of the group) is that of stain_stats_kernel
            int lum[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) lum[i] = tissue_lum(s.ty, rr[i], gg[i], bb[i]);
            unsigned nib = 0;
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                double x[2], y[2], z[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    x[i] = ods[rr[2 * h2 + i] * HCOPY];
                    y[i] = ods[gg[2 * h2 + i] * HCOPY];
                    z[i] = ods[bb[2 * h2 + i] * HCOPY];
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (valid && lum_is_tissue(lum[2 * h2 + i], y_thr)) {
                        nib |= 1u << (2 * h2 + i);
                        od_moments_add(acc, x[i], y[i], z[i]);
                    }
                }
            }
            tmask |= (unsigned long long)nib << (4 * j);
        }
        block_sum_r(acc, s);
        RSTAMP(TM_P2)
        const double nt = acc[0];
        const unsigned long long n_tissue = (unsigned long long)nt;
        if (n_tissue == 0) {
            if (tid == 0) {
                out[TIA_ST_NTISSUE] = 0.0;
                out[TIA_ST_FLAGS] = (double)TIA_FLAG_EMPTY_MASK;
            }
            return;  // uniform across the block
        }
        if (n_tissue < 2) flags |= TIA_FLAG_DEGENERATE;
        if (tid == 0) {
            double cov[6], e1[3], e2[3], mom[10];
            for (int i = 0; i < 10; ++i) mom[i] = acc[i];  // only this lane's copy goes through memory (the callee takes references)
            reg_eigen(mom, cov, e1, e2);
            for (int i = 0; i < 6; ++i) out[TIA_ST_COV + i] = cov[i];
            for (int i = 0; i < 3; ++i) {
                s.bc[2 + i] = e1[i];
                s.bc[5 + i] = e2[i];
                out[TIA_ST_EVEC + i] = e1[i];
                out[TIA_ST_EVEC + 3 + i] = e2[i];
            }
            out[TIA_ST_NTISSUE] = nt;
        }
        __syncthreads();
        RSTAMP(TM_EIG)
        // the eigenvectors stay in LDS (s.bc[2..7]); only the float32 images the sweep needs go to (scalar) registers

        // ---- P3: exact percentiles of phi over the tissue pixels (see stain_stats_kernel for the error budget) ------------------
        unsigned long long kp[2], kn[2], nn[2] = {n_tissue, n_tissue};
        double gm[2];
        np_index(n_tissue, prm.q_phi_lo, kp[0], kn[0], gm[0]);
        np_index(n_tissue, prm.q_phi_hi, kp[1], kn[1], gm[1]);
        double vp[2], vn[2];
        Proj32<Log2Table> proj(s.bc[2], s.bc[3], s.bc[4], s.bc[5], s.bc[6], s.bc[7], Log2Table{s.l2 + (lane & (L2COPY - 1))});
        uni(proj);
        const float tol = angle_tol;
        const bool ok = window_select_reg(
            fetch_sample, hw, true,
            [&](long, uint32_t r, uint32_t g, uint32_t b, float (&v)[2]) -> unsigned {
                if (!is_tissue(s.ty, r, g, b, y_thr)) return 0u;
                float x, y;
                proj(r, g, b, x, y);
                v[0] = v[1] = pseudo_angle32(y, x);
                return 3u;
            },
            [&](uint32_t r, uint32_t g, uint32_t b, double (&x)[2]) {
                const double ox = s.od[r], oy = s.od[g], oz = s.od[b];
                const double p0 = dot3(ox, oy, oz, s.bc[2], s.bc[3], s.bc[4]);
                const double p1 = dot3(ox, oy, oz, s.bc[5], s.bc[6], s.bc[7]);
                x[0] = x[1] = pseudo_angle(p1, p0);
            },
            [&](uint4* seg, unsigned cap, unsigned& count, unsigned& bl0, unsigned& bl1) {
                const double w[4] = {s.ws.wlo[0], s.ws.whi[0], s.ws.wlo[1], s.ws.whi[1]};
                bool edges_ok = true;
#pragma unroll
                for (int i = 0; i < 4; ++i) edges_ok = edges_ok && (!(fabs(w[i]) < 1e300) || fabs(w[i]) <= 1.0);
                const unsigned eok = edges_ok ? 1u : 0u;
                const float lo0 = uni((float)w[0]), hi0 = uni((float)w[1]), lo1 = uni((float)w[2]), hi1 = uni((float)w[3]);
                // all predicates as 0 / 1 integers from sign bits (VALU only: no compare -> scalar mask -> select round trips):
                // below <=> s + tol < 0, above <=> tol - s < 0, plain <=> tol - x < 0; NaNs (an infinite edge times d = 0) can
                // only arise where plain = 0, which masks them
#pragma unroll 1
                for (int j = 0; j < n_slots; ++j) {
                    const unsigned valid = tid + RT * j < ng ? 1u : 0u;
                    uint32_t rr[4], gg[4], bb[4];
                    unpack_group(pa[j], pb[j], pc[j], rr, gg, bb);
                    unsigned fl = 0u;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned tb = (unsigned)(tmask >> (4 * j + i)) & valid;
                        float x, y;
                        proj(rr[i], gg[i], bb[i], x, y);
                        const float d = fabsf(x) + fabsf(y);
                        const unsigned pl = sgn(tol - x) & eok;
                        const unsigned bel0 = sgn(fmaf(-lo0, d, y) + tol), abv0 = sgn(tol - fmaf(-hi0, d, y));
                        const unsigned bel1 = sgn(fmaf(-lo1, d, y) + tol), abv1 = sgn(tol - fmaf(-hi1, d, y));
                        bl0 += tb & pl & bel0;
                        bl1 += tb & pl & bel1;
                        const unsigned dec0 = pl & (bel0 | abv0), dec1 = pl & (bel1 | abv1);
                        fl |= ((tb & (dec0 ^ 1u)) | ((tb & (dec1 ^ 1u)) << 1)) << (2 * i);
                    }
                    seg_push(fl != 0u, make_uint4(pa[j], pb[j], pc[j], fl), seg, cap, count);
                }
            },
            s, kp, nn, vp, vn);
        if (!ok) {
            give_up();
            return;
        }
        if (tid == 0) {
            const double e1[3] = {s.bc[2], s.bc[3], s.bc[4]}, e2[3] = {s.bc[5], s.bc[6], s.bc[7]};
            double phi[2], hv[3], ev[3];
            reg_stain_from_angles(vp, vn, gm, e1, e2, phi, hv, ev);
            out[TIA_ST_MINPHI] = phi[0];
            out[TIA_ST_MAXPHI] = phi[1];
            for (int i = 0; i < 3; ++i) {
                s.bc[8 + i] = hv[i];
                s.bc[11 + i] = ev[i];
            }
        }
    } else {
        if (tid == 0)
            for (int i = 0; i < 6; ++i) s.bc[8 + i] = prm.mode == TIA_MODE_GIVEN ? s_given[i] : prm.stain_fixed[i];
    }

#if TIA_STATS_TIMING
    if (tid == 0) s.tm[TM_PHI_TOTAL] = clock64() - t_begin;
#endif
    // ---- pseudo-inverse (stain matrix S = s.bc[8..13], P = s.bc[14..19]: both stay in LDS) ---------------------------------------
    if (tid == 0) {
        double P[6];
        stats_pinv(&s.bc[8], P);
        for (int i = 0; i < 6; ++i) s.bc[14 + i] = P[i];
    }
    __syncthreads();
    const double* P = &s.bc[14];

    // ---- P4: exact percentile of both concentration channels over ALL pixels ----------------------------------------------------
    double maxc[2];
    {
        const unsigned long long npx = (unsigned long long)hw;
        unsigned long long kp[2], kn[2], nn[2] = {npx, npx};
        double gm[2];
        np_index(npx, prm.q_conc, kp[0], kn[0], gm[0]);
        kp[1] = kp[0];
        kn[1] = kn[0];
        gm[1] = gm[0];
        double vp[2], vn[2];
        Proj32<Log2Table> conc32(P[0], P[2], P[4], P[1], P[3], P[5], Log2Table{s.l2 + (lane & (L2COPY - 1))});
        uni(conc32);
        const float tol0 = uni(conc_tol(P[0], P[2], P[4])), tol1 = uni(conc_tol(P[1], P[3], P[5]));
        const bool ok = window_select_reg(
            fetch_sample, hw, false,
            [&](long, uint32_t r, uint32_t g, uint32_t b, float (&v)[2]) -> unsigned {
                conc32(r, g, b, v[0], v[1]);
                return 3u;
            },
            [&](uint32_t r, uint32_t g, uint32_t b, double (&x)[2]) {
                const double ox = s.od[r], oy = s.od[g], oz = s.od[b];
                x[0] = dot3(ox, oy, oz, P[0], P[2], P[4]);  // P read from LDS at the point of use
                x[1] = dot3(ox, oy, oz, P[1], P[3], P[5]);
            },
            [&](uint4* seg, unsigned cap, unsigned& count, unsigned& bl0, unsigned& bl1) {
                const float lo0 = uni((float)s.ws.wlo[0]), hi0 = uni((float)s.ws.whi[0]), lo1 = uni((float)s.ws.wlo[1]), hi1 = uni((float)s.ws.whi[1]);
                const float t0 = uni(tol0 + edge_slack(lo0) + edge_slack(hi0)), t1 = uni(tol1 + edge_slack(lo1) + edge_slack(hi1));
                // below <=> (c + t) - lo < 0, above <=> hi - (c - t) < 0 (differences of finite / infinite floats: never NaN here)
#pragma unroll 1
                for (int j = 0; j < n_slots; ++j) {
                    const unsigned valid = tid + RT * j < ng ? 1u : 0u;
                    uint32_t rr[4], gg[4], bb[4];
                    unpack_group(pa[j], pb[j], pc[j], rr, gg, bb);
                    unsigned fl = 0u;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float c0, c1;
                        conc32(rr[i], gg[i], bb[i], c0, c1);
                        const unsigned bel0 = sgn((c0 + t0) - lo0), abv0 = sgn(hi0 - (c0 - t0));
                        const unsigned bel1 = sgn((c1 + t1) - lo1), abv1 = sgn(hi1 - (c1 - t1));
                        bl0 += valid & bel0;
                        bl1 += valid & bel1;
                        fl |= ((valid & ((bel0 | abv0) ^ 1u)) | ((valid & ((bel1 | abv1) ^ 1u)) << 1)) << (2 * i);
                    }
                    seg_push(fl != 0u, make_uint4(pa[j], pb[j], pc[j], fl), seg, cap, count);
                }
            },
            s, kp, nn, vp, vn);
        if (!ok) {
            give_up();
            return;
        }
        maxc[0] = np_lerp(vp[0], vn[0], gm[0]);
        maxc[1] = np_lerp(vp[1], vn[1], gm[1]);
    }

    if (tid == 0) {
        stats_finish_record(out, prm, &s.bc[8], P, maxc, flags);
#if TIA_STATS_TIMING
        s.tm[TM_TOTAL] = clock64() - t_begin;
        s.tm[TM_CONC_TOTAL] = s.tm[TM_TOTAL] - s.tm[TM_PHI_TOTAL];
        for (int i = 0; i < 16; ++i) out[TIA_ST_CYCLES + i] = (double)s.tm[i];
#endif
    }
}

long stain_stats_reg_pixel_limit() { return (long)RT * RG * 4; }

int launch_stain_stats_reg(const uint8_t* d_img, long n, long hw, const tia_stain_tables* d_tables, const tia_stain_params& prm,
                           double* d_stats, int* redo, uint32_t* ws, hipStream_t st) {
    static DeviceOnce attr_once;  // the dynamic-LDS attribute is per device
    if (!attr_once.ensure([] {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(&stain_stats_reg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)sizeof(SmemR)) == hipSuccess;
        }))
        return TIA_ELAUNCH;
    hipLaunchKernelGGL(stain_stats_reg_kernel, dim3((unsigned)n), dim3(RT), sizeof(SmemR), st, d_img, hw, d_tables, prm, d_stats, redo, ws);
    return hipGetLastError() == hipSuccess ? TIA_OK : TIA_ELAUNCH;
}

}  // namespace tia
