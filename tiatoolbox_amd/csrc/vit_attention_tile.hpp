// The one copy of what the half-precision attention kernels share: mha_fwd_h_kernel (vit_attention.hip) and
// mha_probs_kernel (vit_attention_maps.hip) are built from these pieces -- mma16, the geometry per head_dim, the workgroup decode, the Q
// load, the staging of a key tile (with or without V), the score tile and the online maximum -- so the maps describe the computation
// that ran by construction.  Layout and arithmetic are described in vit_attention.hip.  The host-side argument check is also
// vit_f32.hip's.
#pragma once
#include "conv_device.hpp"
#include "wide_io.hpp"

namespace tia {
namespace mha {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int AT = 256;      // threads: 4 waves x 16 query rows
constexpr int KV_TILE = 64;  // keys per LDS tile

// What tia_mha_fwd_h, tia_mha_probs_h / _fused_h and tia_mha_fwd_f32 refuse alike, in this order.  q_rows: the queries computed per
// (image, head) (s for a forward); groups: workgroups per (image, query tile) -- heads, or 1 where one workgroup owns every head.
inline int check_args(const void* d_qkv, const void* d_out, int64_t n, int64_t s, int64_t heads, int64_t head_dim, float scale, bool dtype_ok,
                      int64_t q_rows, int64_t groups, long* q_tiles) {
    if (!d_qkv || !d_out || n <= 0 || s <= 0 || heads <= 0 || head_dim <= 0) return TIA_EINVAL;
    if (!dtype_ok) return TIA_EINVAL;
    if (!(scale > 0.0f) || !(scale < INFINITY)) return TIA_EINVAL;
    if (head_dim != 64 && head_dim != 80) return TIA_ESIZE;
    if ((reinterpret_cast<uintptr_t>(d_qkv) | reinterpret_cast<uintptr_t>(d_out)) & 15) return TIA_EINVAL;
    if (s > 0x7fffffffL - KV_TILE || heads > 0x7fffffffL / (3 * head_dim)) return TIA_ESIZE;
    *q_tiles = (q_rows + 63) / 64;
    if (n > 0x7fffffffL / groups || n * groups > 0x7fffffffL / *q_tiles) return TIA_ESIZE;  // one grid dimension
    return TIA_OK;
}

template <bool BF>
__device__ __forceinline__ f32x4 mma16(const v4u& a, const v4u& b, const f32x4& c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const b8*>(&a), *reinterpret_cast<const b8*>(&b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(&a), *reinterpret_cast<const h8*>(&b), c, 0, 0, 0);
}

// ---- geometry per head_dim ----------------------------------------------------------------------------------------------------------
// HD 64: two k-steps of the 16x16x32 MFMA, LDS rows of 64 + 8 halves (144 bytes: 16-byte aligned, 16-byte reads of 16 rows spread over
// the banks), a tile of 64 rows x 8 sixteen-byte vectors = 2 per thread.
// HD 80 (Virchow / Virchow2: 1280 / 16):
//  * First product: k = 80 is 2.5 steps, run as three whose dims 80..95 are exact zeros in BOTH operands.  Those dims are lane quarters
//    2 and 3 of step 2.  For Q such a lane keeps a zero register; for K it reads a real address (the row's dims 64 + 8 (quarter & 1), so
//    that every lane of the wave issues the same read) and then SUBSTITUTES the zero register: no LDS pad column exists, so none can
//    hold stale or uninitialised bits (0 x NaN would be NaN), and LDS has no 96-wide rows to pay for.
//  * Second product: 80 output dims are five 16-row blocks, no padding; the transposed V image has 80 rows (slots 64..79 unused).
//  * A tile is 64 rows x 10 vectors per operand = 640 = 2.5 per thread: three staging rounds, the last one guarded.
//  * LDS row pitch 80 halves (160 bytes).  ds_read_b128 banks are (byte address / 4) mod 64 and conflicts count inside four 16-lane
//    groups, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: a group holds rows {0-3, 12-15} of one lane quarter and rows
//    {4-11} of the next, all 16 rows once.  In 16-byte slots (16 per 256-byte bank row) lane (row r, quarter q) reads slot
//    (10 r + q + 4 step) mod 16: 10 r mod 16 is {0, 10, 4, 14} for r = 0..3 and {8, 2, 12, 6} for r = 12..15 -- the eight even slots --
//    and for r = 4..11 the eight even slots again, which the next quarter's + 1 makes the eight odd ones: 16 distinct slots, no
//    conflict, in either kind of group and at every step (the substituted lanes of step 2 read quarter & 1, the same picture).  A pitch
//    of 72 or 88 (+ 8 halves of pad, the 64 form's habit) is 2-way by the same count, 80 and 112 are free; 80 needs no pad.
template <int HD>
struct Geo {
    static_assert(HD == 64 || HD == 80, "head_dim 64 or 80");
    static constexpr int PITCH = HD == 64 ? 72 : 80;               // halves per LDS row
    static constexpr int FULL_STEPS = HD / 32;                     // k-steps whose 32 dims are all real
    static constexpr int STEPS = (HD + 31) / 32;                   // ... and the half-real one of HD 80
    static constexpr int VEC = HD / 8;                             // 16-byte vectors per row
    static constexpr int ROUNDS = (KV_TILE * VEC + AT - 1) / AT;   // staging rounds of the workgroup
    static constexpr bool WHOLE_ROUNDS = KV_TILE * VEC % AT == 0;  // every round moves a vector per thread: no guard
    static constexpr int BLOCKS = HD / 16;                         // 16-dim blocks of an output row
};

// ---- workgroup decode ---------------------------------------------------------------------------------------------------------------
// blockIdx.x = rest * q_tiles + query tile; what `rest` numbers -- (image, head), or the image alone -- is its kernel's business
struct Where {
    int tid, lane, wave, r16, quarter;
    int qt, query;  // the 64-query tile, and this lane's query: 64 qt + 16 wave + (lane & 15)
    long rest;
};

__device__ __forceinline__ Where decode(int q_tiles) {
    Where w;
    w.tid = threadIdx.x, w.lane = w.tid & 63, w.wave = w.tid >> 6;
    w.r16 = w.lane & 15, w.quarter = w.lane >> 4;
    const long bid = blockIdx.x;
    w.qt = (int)(bid % q_tiles);
    w.rest = bid / q_tiles;
    w.query = w.qt * 64 + w.wave * 16 + w.r16;
    return w;
}

// ---- Q: the B operand, dims 32 step + 8 quarter .. + 7 of the lane's query; zeros for queries >= q_rows and for dims >= HD ----------
template <int HD>
__device__ __forceinline__ void load_q(const unsigned short* base, long row_stride, int query, int q_rows, int quarter,
                                       v4u (&qf)[Geo<HD>::STEPS]) {
    const v4u zero4 = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int st = 0; st < Geo<HD>::STEPS; ++st) {
        const bool real = query < q_rows && 32 * st + 8 * quarter < HD;
        qf[st] = real ? *reinterpret_cast<const v4u*>(base + (long)query * row_stride + 32 * st + 8 * quarter) : zero4;
    }
}

// where key `row` of a tile sits in a row of the transposed V image: the k order of the P^T operand (vit_attention.hip)
__device__ __forceinline__ int key_slot(int row) {
    const int kk = row & 31;
    return (row & 32) + 8 * ((kk >> 2) & 3) + 4 * (kk >> 4) + (kk & 3);
}

// ---- staging: keys k0 .. k0 + 63 of one head into k_lds ([key][dim]) and -- WITH_V -- their values into vt_lds ([dim][key slot]), zeros
// beyond s.  Vector idx of the tile is row idx / VEC, dims 8 (idx % VEC) .. + 7; a thread moves vectors tid, tid + 256, ...  All global
// loads are issued before the first barrier, and both barriers of a tile are in here.
template <int HD, bool WITH_V>
__device__ __forceinline__ void stage_tile(const unsigned short* kbase, const unsigned short* vbase, long row_stride, int k0, int s, int tid,
                                           unsigned short* k_lds, unsigned short* vt_lds) {
    using G = Geo<HD>;
    const v4u zero4 = {0u, 0u, 0u, 0u};
    v4u kreg[G::ROUNDS];
    [[maybe_unused]] v4u vreg[G::ROUNDS];
#pragma unroll
    for (int i = 0; i < G::ROUNDS; ++i) {
        const int idx = tid + AT * i, row = idx / G::VEC, c = idx - row * G::VEC, key = k0 + row;
        const long off = (long)key * row_stride + 8 * c;
        const bool real = (G::WHOLE_ROUNDS || idx < KV_TILE * G::VEC) && key < s;
        kreg[i] = real ? *reinterpret_cast<const v4u*>(kbase + off) : zero4;
        if constexpr (WITH_V) vreg[i] = real ? *reinterpret_cast<const v4u*>(vbase + off) : zero4;
    }
    __syncthreads();  // every wave has finished reading the previous tile
#pragma unroll
    for (int i = 0; i < G::ROUNDS; ++i) {
        const int idx = tid + AT * i, row = idx / G::VEC, c = idx - row * G::VEC;
        if (G::WHOLE_ROUNDS || idx < KV_TILE * G::VEC) {  // (a constant where the rounds are whole: HD 64 stages unguarded)
            *reinterpret_cast<v4u*>(&k_lds[row * G::PITCH + 8 * c]) = kreg[i];
            if constexpr (WITH_V) {
                const int slot = key_slot(row);
                const unsigned w[4] = {vreg[i].x, vreg[i].y, vreg[i].z, vreg[i].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    vt_lds[(8 * c + 2 * e) * G::PITCH + slot] = (unsigned short)(w[e] & 0xffffu);
                    vt_lds[(8 * c + 2 * e + 1) * G::PITCH + slot] = (unsigned short)(w[e] >> 16);
                }
            }
        }
    }
    __syncthreads();
}

// ---- scores: S^T = K Q^T, 4 key groups x STEPS k-steps; t[kt][r] = scale * log2 e * score(query l & 15, key k0 + 16 kt + 4 quarter + r),
// -inf for keys >= s.  Returns the maximum of the lane's 16 values (15 register operations; online_max exchanges it).
template <bool BF, int HD>
__device__ __forceinline__ float score_tile(const unsigned short* k_lds, const v4u (&qf)[Geo<HD>::STEPS], int k0, int s, int r16, int quarter,
                                            float scale_log2e, f32x4 (&t)[4]) {
    using G = Geo<HD>;
    const v4u zero4 = {0u, 0u, 0u, 0u};
    const bool pad_lane = quarter >= 2;  // HD 80: dims 80..95 of step 2 (see Geo); no step of HD 64 is a pad step
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int st = 0; st < G::STEPS; ++st) {
            const bool pad_step = st >= G::FULL_STEPS;
            const int col = pad_step ? 32 * st + 8 * (quarter & 1) : 32 * st + 8 * quarter;  // (always inside the row's HD dims)
            v4u a = *reinterpret_cast<const v4u*>(&k_lds[(16 * kt + r16) * G::PITCH + col]);
            if (pad_step && pad_lane) a = zero4;
            acc = mma16<BF>(a, qf[st], acc);
        }
        t[kt] = acc;
    }
    float t_max = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + 16 * kt + 4 * quarter + r;
            const float v = key < s ? t[kt][r] * scale_log2e : -INFINITY;
            t[kt][r] = v;
            t_max = fmaxf(t_max, v);
        }
    return t_max;
}

// ---- online softmax, base-2 domain: two lane exchanges finish the tile maximum of a query (t_max: the lane's own, from score_tile);
// m_run moves to the new maximum and alpha = exp2(m_old - m_new) is returned.  What follows stays at the two call sites, in this shape:
//     p = exp2(t[kt][r] - m_run), p_sum += p in (kt, r) order, l_run = l_run * alpha + p_sum
// (l_run: this lane's share of the row sum, its 16 keys per tile).  As part of this helper the compiler parts the additions from the
// exponentials (an instruction order, not a value), and the fp16 head_dim-80 forward ran 4 % longer (profiles/attention_one_copy_perf.txt).
__device__ __forceinline__ float online_max(float t_max, float& m_run) {
    t_max = fmaxf(t_max, __shfl_xor(t_max, 16, 64));
    t_max = fmaxf(t_max, __shfl_xor(t_max, 32, 64));
    const float m_new = fmaxf(m_run, t_max);                    // finite: the tile holds a real key
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // first tile: exp2(-inf) = 0
    m_run = m_new;
    return alpha;
}

// a query's row sum from its four lanes' shares
__device__ __forceinline__ float row_sum(float l_run) {
    float l_tot = l_run + __shfl_xor(l_run, 16, 64);
    l_tot += __shfl_xor(l_tot, 32, 64);
    return l_tot;
}

}  // namespace mha
}  // namespace tia
