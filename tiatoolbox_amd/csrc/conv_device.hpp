// Device leaves shared by the convolution kernels (conv3x3_wino.hip, conv3x3_wino42.hip, conv3x3_spatial.hip, conv_mfma.hip,
// conv_mfma_h.hip, conv_ring_bf16x3.hip, conv3x3_wino_bf16x3.hip, stem_mfma.hip) and the half-precision glue (cnn_epilogue_h.hip); internal, not part of
// the C ABI.  Every device function here is a __forceinline__ leaf over scalars, and only what leaves the kernels' instruction
// streams as they were is shared (profiles/conv_gemm_refactor_isa.txt; DESIGN 4.28 says what could not be).  The kernels keep
// their own helpers in anonymous namespaces and say `using namespace tia;` inside them.  The host side of the implicit-GEMM
// kernels is conv_host.hpp (device_cu_count, at the bottom here, is the host leaf every kernel file already reaches this way).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace tia {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using h8 = __attribute__((ext_vector_type(8))) _Float16;
using b8 = __attribute__((ext_vector_type(8))) __bf16;

// Operands come through buffer descriptors (built from kernel arguments only, so they live in SGPRs): a 32-bit per-lane byte
// offset is all the address arithmetic a load needs, and an out-of-range offset reads as zero -- which is exactly what a padding
// tap must contribute, without a select after the load.
constexpr int OOB = (int)0x80000000;           // voffset beyond every buffer extent: the load returns zeros (padding taps)
constexpr int kBufferRsrcFlags = 0x00020000;   // descriptor word 3 of a raw buffer: DATA_FORMAT = 32 (bits 18:15 = 4), every other field zero

// 16 bytes per lane from a buffer straight into LDS (buffer_load_dwordx4 ... lds): the wave's 64 lanes fill the 1 KB at
// `lds_wave_base` in lane order; an out-of-range `voffset` writes zeros.  (A __device__ function: the builtin must not be seen by
// the host pass, which otherwise drops the kernel's launch stub.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lds_wave_base, int voffset, int soffset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voffset, soffset, 0, 0);
}

// s_waitcnt vmcnt(VM) lgkmcnt(0) (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] = 7 (no wait) | lgkmcnt[11:8] | vmcnt[5:4] << 14)
template <int VM>
__device__ __forceinline__ void wait_vm_lgkm0() {
    __builtin_amdgcn_s_waitcnt((VM & 15) | (7 << 4) | ((VM >> 4) << 14));
    asm volatile("" ::: "memory");
}

// Packed float32 add / subtract (two channels per instruction).  Inline assembly: the compiler splits a v2f32 subtraction into two
// scalar v_sub_f32 (48 of the 56 vector instructions of a load phase of the F(2x2) Winograd kernel), and it is the NUMBER of vector
// instructions issued beside the SIMD partner's MFMA stream that stretches that phase.
__device__ __forceinline__ f32x2 pk_add(f32x2 a, f32x2 b) {
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
    f32x2 r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// ---- the three-part bf16 split of a float32 operand in registers (conv_ring_bf16x3.hip, conv3x3_wino_bf16x3.hip) ----

using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

// two float32 -> two bf16 (round to nearest even) in one register: v_cvt_pk_bf16_f32; element 0 in the low half
__device__ __forceinline__ unsigned cvt_pk_bf16(float v0, float v1) {
    const bf16x2 p = __builtin_convertvector(f32x2{v0, v1}, bf16x2);
    unsigned r;
    __builtin_memcpy(&r, &p, 4);
    return r;
}

// a - b as ONE v_sub_f32.  Inline assembly: left to itself the compiler pairs the split's subtractions into v_pk_add_f32, and a
// packed float32 instruction beside the MFMA stream costs more than the two plain ones it replaces (pk_add / pk_sub above are the
// opposite case).  The arithmetic is the same IEEE subtraction either way.
__device__ __forceinline__ float sub_f32(float a, float b) {
    float r;
    asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// a + b as ONE v_add_f32 (the same reason)
__device__ __forceinline__ float add_f32(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// (v0, v1) -> packed hi, mid, lo with v = hi + mid + lo exactly; the subtractions are plain float32 subtractions of a value and
// its own rounding (exact: the difference has at most 16, then 8, significant bits)
__device__ __forceinline__ void split_pair(float v0, float v1, unsigned& ph, unsigned& pm, unsigned& pl) {
    ph = cvt_pk_bf16(v0, v1);
    const float r0 = sub_f32(v0, __uint_as_float(ph << 16)), r1 = sub_f32(v1, __uint_as_float(ph & 0xffff0000u));
    pm = cvt_pk_bf16(r0, r1);
    const float s0 = sub_f32(r0, __uint_as_float(pm << 16)), s1 = sub_f32(r1, __uint_as_float(pm & 0xffff0000u));
    pl = cvt_pk_bf16(s0, s1);
}

// v_mfma_f32_32x32x16_bf16: a lane holds row (column) lane & 31, k = 8 (lane >> 5) .. + 7 of A (B) as eight bf16 in four registers
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const b8*>(&a), *reinterpret_cast<const b8*>(&b), c, 0, 0, 0);
}

// The Winograd kernels' LDS patch rows, in 16-byte units: pixels are stored in PAIRS of 9 units (two pixels of 4 units + one padding
// unit; the bank analysis is in conv3x3_wino.hip).  Unit offset of pixel column px inside a row:
__device__ __forceinline__ constexpr int px_unit(int px) { return (px >> 1) * 9 + (px & 1) * 4; }

// float16 (BF = false) / bfloat16 (BF = true) bits <-> float32.  bfloat16 NaN rule: a NaN keeps its sign and upper payload and gets
// the quiet bit -- the rounding increment would carry a NaN with a full low payload into infinity or the sign.
template <bool BF>
__device__ __forceinline__ float half_to_f32(unsigned short v) {
    if constexpr (BF) return __uint_as_float((unsigned)v << 16);
    _Float16 h;
    __builtin_memcpy(&h, &v, 2);
    return (float)h;
}
template <bool BF>
__device__ __forceinline__ unsigned short f32_to_half(float x) {  // round to nearest even
    if constexpr (BF) {
        unsigned u = __float_as_uint(x);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (unsigned short)(u >> 16);
    } else {
        const _Float16 h = (_Float16)x;
        unsigned short v;
        __builtin_memcpy(&v, &h, 2);
        return v;
    }
}

// ---- the tile order of every convolution kernel, and what the implicit-GEMM kernels that gather kh x kw taps share (conv_mfma.hip,
//      conv_mfma_h.hip, conv1x1_ring_kernel in conv3x3_spatial.hip, conv_ring_bf16x3.hip) --------------------------------------------

// XCD-aware tile order: workgroups go round-robin to the 8 XCDs (each with its own L2); every XCD gets a contiguous range of
// xcd_share() pixel tiles (neighbouring tiles share their input halo rows).  The grid is whole rounds over the XCDs: a workgroup
// whose xcd_tile() is >= m_tiles has no tile and leaves.  (A form that returns a negative index instead tells the compiler that
// the index of the others is non-negative, and every kernel's prologue comes out different: measured)
__device__ __forceinline__ int xcd_share(int m_tiles) { return (m_tiles + 7) / 8; }
__device__ __forceinline__ int xcd_tile(int bid, int m_tiles) {
    const int per_xcd = xcd_share(m_tiles);
    return (bid % 8) * per_xcd + bid / 8;
}

// Slice cursor (scalar): tap (kh, kw) and channel position c of the slice that is requested next.  next() advances the channel
// position by `step` up to `c_end` (in channels: BK against cin; or in slices: 1 against cin / 16), then the tap column, then the tap
// row; past the last slice the cursor stays there (the tail of a pipeline re-requests the last slice, so its loop body has no
// control flow around the loads).
struct SliceCursor {
    int kh = 0, kw = 0, c = 0;
    __device__ __forceinline__ void next(int step, int c_end, int n_kh, int n_kw) {
        int c2 = c + step, kw2 = kw, kh2 = kh;
        if (c2 == c_end) { c2 = 0; ++kw2; }
        if (kw2 == n_kw) { kw2 = 0; ++kh2; }
        if (kh2 < n_kh) { c = c2; kw = kw2; kh = kh2; }
    }
};

// Dimensions of a launch of the ring kernels (conv1x1_ring_kernel, conv_ring_bf16x3_kernel)
struct PwDims {
    int n, h, w, cin, cout, ho, wo, stride;
    unsigned x_bytes, w_bytes;
    int kh, kw, pad_y, pad_x;
};

// Compute units of the calling thread's CURRENT device (MI355X: 256), cached per device index (a process may drive several GPUs;
// the first caller may be a host-only route query).  Without a usable device (build container): MI355X's 256.
inline long device_cu_count() {
    static std::atomic<int> cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int cus = cached[dev].load(std::memory_order_relaxed);
    if (cus == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
        cached[dev].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

}  // namespace tia
