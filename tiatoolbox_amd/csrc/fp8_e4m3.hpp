// OCP e4m3fn codes (largest finite value 448, no infinities, 0x7f / 0xff NaN; NOT the MI300 fnuz encoding) from float32: round to
// nearest even, saturating at +-448 -- torch's CPU `.to(torch.float8_e4m3fn)` on finite inputs of magnitude <= 464, and 448 beyond.
// Integer arithmetic on the float32 bits, so the host and the device give the same code for every input (vit_fp8.hip; internal, not
// part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

namespace tia {

__host__ __device__ __forceinline__ unsigned f32_to_e4m3(float x) {
    const unsigned sign = (__builtin_bit_cast(unsigned, x) >> 24) & 0x80u;
    float a = __builtin_fabsf(x);
    a = a < 448.0f ? a : 448.0f;  // saturation (a NaN saturates as well: the producers never make one from finite rows)
    unsigned code;
    if (a < 0.015625f) {
        // below the smallest normal 2^-6 the codes 0 .. 7 step by 2^-9; a * 512 is exact, rint rounds to nearest even, and 8 is
        // the code of 2^-6 itself
        code = (unsigned)__builtin_rintf(a * 512.0f);
    } else {
        unsigned v = __builtin_bit_cast(unsigned, a);
        v += 0x7ffffu + ((v >> 20) & 1u);  // to 3 mantissa bits, ties to even; a carry moves into the exponent
        code = (v >> 20) - (120u << 3);    // exponent bias 127 -> 7
    }
    return sign | code;
}

}  // namespace tia
