// vk_exactdiv.hpp -- the f32 divisions of the cell march's ray set-up (vk_march_kernel_body.hpp) without the generic expansion.
//
// For `a / b` in binary32 the compiler emits ten instructions:
//     bs = v_div_scale_f32(b, b, a);  as = v_div_scale_f32(a, b, a)  [sets VCC];  y0 = v_rcp_f32(bs);
//     e = fma(-bs, y0, 1);  y = fma(e, y0, y0);  q0 = as * y;  r0 = fma(-bs, q0, as);  q1 = fma(r0, y, q0);  r1 = fma(-bs, q1, as);
//     q = v_div_fmas_f32(r1, y, q1)  [fma, times 2^+-32 under VCC];  v_div_fixup_f32(q, b, a)
// The three v_div_* instructions exist for operands near the ends of the exponent range and for zeros, infinities and NaNs.  From their
// definitions in the CDNA ISA reference (exponent() is the biased exponent field):
//     v_div_scale_f32 S0, S1 = b, S2 = a   returns S0 unchanged with VCC = 0 unless one of these holds:  a == 0 or b == 0;
//         exponent(a) - exponent(b) >= 96;  b is subnormal;  1 / b is subnormal (|b| > 2^126);  a / b is subnormal;  exponent(a) <= 23 (|a| < 2^-103)
//     v_div_fmas_f32                       is fma(S0, S1, S2) while VCC = 0
//     v_div_fixup_f32 S0 = q, S1 = b, S2 = a   returns q with the sign of a xor b unless one of these holds:  a or b is a NaN, an infinity or a zero;
//         exponent(a) - exponent(b) < -150 or >= 128;  exponent(b) == 255
// kDivLo <= |a|, |b| <= kDivHi (2^-40 .. 2^40) is far inside all of them: exponents differ by at most 80, a / b >= 2^-80 and 1 / b >= 2^-40 are normal, q is
// finite and carries the quotient's sign already.  For such operands div_inrange below is, instruction for instruction on the same values, what the
// expansion executes -- the same bits by construction, whatever v_rcp_f32 returns.  The same holds for 1 / b with 2^-81 <= |b| <= 2^40 (kRcpLo, kRcpHi:
// the direction components behind a guarded normalisation -- at least kDivLo / kDivHi, rounded once -- and their products with a volume dimension).
//
// recip_refine / div_by: the three instructions that depend on b alone (y0, e, y) once per divisor, five per quotient.
// div_const: b is a constant of the launch and y = RN(1 / b) comes from the host; q0 = a y, q = fma(fma(-b, q0, a), y, q0).  Not the
//     expansion's chain: equal to RN(a / b) for the operands it is used on -- a = 2 (x + 0.5), b = W, x < W <= kDivConstMax -- by exhaustive
//     check (tests/exactdiv_fuzz.cpp on the host, tests/exactdiv_device.hip against the device's own division).
// pow2_recip: 1 / p for a power of two, by exponent arithmetic.  1 / (p |d|) == |1 / d| (1 / p) in binary32: every step of the chain scales exactly.
//
// The core functions take the reciprocal's seed as an argument (on the device it is v_rcp_f32, accurate to 1 ulp): tests/exactdiv_fuzz.cpp feeds
// them both neighbours of the true 1 / b.  No HIP needed: tests/test_exactdiv_cpu.py builds that program with plain g++ under sanitizers.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VK_HD __host__ __device__ __forceinline__
#else
#define VK_HD inline
#endif

namespace vk {

constexpr float kDivLo = 0x1p-40f, kDivHi = 0x1p40f;  // |numerator|, |divisor| of div_inrange / div_by
constexpr float kRcpLo = 0x1p-81f, kRcpHi = 0x1p40f;  // |divisor| of div_inrange(1, b)
constexpr uint32_t kDivConstMax = 16384;              // div_const: image sizes checked exhaustively

struct Recip { float b, y; };  // a divisor and its refined reciprocal

VK_HD Recip recip_refine_seeded(float b, float y0) {
    const float e = fmaf(-b, y0, 1.0f);
    return Recip{b, fmaf(e, y0, y0)};
}
VK_HD float div_by(float a, Recip r) {
    const float q0 = a * r.y;
    const float r0 = fmaf(-r.b, q0, a);
    const float q1 = fmaf(r0, r.y, q0);
    const float r1 = fmaf(-r.b, q1, a);
    return fmaf(r1, r.y, q1);
}
VK_HD float div_inrange_seeded(float a, float b, float y0) { return div_by(a, recip_refine_seeded(b, y0)); }

VK_HD float div_const(float a, float b, float y) {
    const float q0 = a * y;
    return fmaf(fmaf(-b, q0, a), y, q0);
}

// 1 / p for p = 2^k, -126 <= k <= 126
VK_HD float pow2_recip(float p) {
    uint32_t u;
    memcpy(&u, &p, 4);
    u = 0x7f000000u - u;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
VK_HD bool is_pow2(uint32_t n) { return n != 0u && (n & (n - 1u)) == 0u; }

#if defined(__HIPCC__)
__device__ __forceinline__ Recip recip_refine(float b) { return recip_refine_seeded(b, __builtin_amdgcn_rcpf(b)); }
__device__ __forceinline__ float div_inrange(float a, float b) { return div_by(a, recip_refine(b)); }
#endif

}  // namespace vk
