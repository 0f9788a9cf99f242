// OCP e4m3fn codes and the power-of-two row scale of mode fp8, in plain integer / fp32 arithmetic that the host and the device compile alike:
// fp8_snap_kernel (gemv_fp8.hip) quantises with these, sonicscribe_amd/fp8.py is their numpy statement.
#pragma once
#include <stdint.h>
#include <string.h>
#if defined(__HIPCC__)
#define FP8_HD __host__ __device__ __forceinline__
#else
#define FP8_HD inline
#endif

#define FP8_E4M3_MAX 448.0f
#define FP8_SCALE_EXP_MIN (-117)      // s >= 2^-117: s times the smallest e4m3 step (2^-9) is still a normal bf16

FP8_HD uint32_t fp8_f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
FP8_HD float fp8_u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
FP8_HD float fp8_pow2(int e) { return fp8_u2f((uint32_t)(e + 127) << 23); }      // e in -126 .. 127

// the exponent e of the smallest power of two s = 2^e with amax / s <= 448 (amax finite, >= 0), clamped below at FP8_SCALE_EXP_MIN; 0 for an all-zero row.
// amax = m 2^x with m in [1, 2): 448 = 1.75 * 2^8, so e = x - 8 when m <= 1.75 and x - 7 above it - amax / s then lies in (224, 448]
FP8_HD int fp8_scale_exp(float amax) {
    const uint32_t u = fp8_f2u(amax) & 0x7fffffffu;
    if (u == 0) return 0;
    const int x = (int)(u >> 23) - 127;                   // (a denormal amax reads as x = -127: clamped below anyway)
    const int e = x - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
    return e < FP8_SCALE_EXP_MIN ? FP8_SCALE_EXP_MIN : e;
}
// round-to-nearest-even of v (|v| <= 448, finite) to e4m3fn: sign | 4 exponent bits (bias 7) | 3 mantissa bits; below 2^-6 the subnormal grid of step 2^-9
FP8_HD uint32_t fp8_encode(float v) {
    const uint32_t u = fp8_f2u(v), sign = (u >> 24) & 0x80u;
    uint32_t a = u & 0x7fffffffu;
    if (a < 0x3c800000u) {                                // |v| < 2^-6: |v| * 512 to the nearest integer, ties to even; 8 carries into the first normal code
        const float t = fp8_u2f(a) * 512.0f;
        uint32_t q = (uint32_t)t;
        const float r = t - (float)q;
        if (r > 0.5f || (r == 0.5f && (q & 1u))) ++q;
        return sign | q;
    }
    a += 0x7ffffu + ((a >> 20) & 1u);                     // RNE at mantissa bit 20 (the carry moves the exponent by itself)
    const uint32_t code = (((a >> 23) - 120u) << 3) | ((a >> 20) & 7u);
    return sign | (code > 0x7eu ? 0x7eu : code);          // (448 is the largest magnitude a snapped row holds; saturate beyond it, never the NaN code)
}
FP8_HD float fp8_decode(uint32_t c) {
    const uint32_t E = (c >> 3) & 15u, m = c & 7u;
    const float a = E ? (float)(8u + m) * fp8_pow2((int)E - 10) : (float)m * 0.001953125f;
    return (c & 0x80u) ? -a : a;
}
