// exactdiv_fuzz.cpp -- vokselis_amd/csrc/vk_exactdiv.hpp on the CPU, under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_exactdiv_cpu.py builds and runs it with plain g++).
//
//   chain    div_inrange_seeded and recip_refine_seeded + div_by against IEEE a / b, the seed taken as EACH of the two floats that bracket the
//            true 1 / b (v_rcp_f32 is accurate to 1 ulp: it returns one of them): every mantissa of b at one exponent with a = 1 (the
//            reciprocals) and with a random numerator, and 50 M random pairs with |a|, |b| in [kDivLo, kDivHi], either sign.  On the device the
//            chain is the compiler's own and needs no such proof (vk_exactdiv.hpp); this says that the chain is also the correctly rounded
//            quotient.  A case in which only the bracket FARTHER from 1 / b differs is seed-dependent: it is listed, and what the device's seed does
//            with it is settled on the device (tests/exactdiv_device.hip).  Known: 1 / 0x1.fffffep0 with the seed 0.5 (the true reciprocal lies
//            just above 0.5, whose other neighbour is 2^-24 away).  Any other difference fails.
//   const    div_const(2 (x + 0.5), W, RN(1 / W)) == 2 (x + 0.5) / W for every x < W <= 16384.
//   pow2     1 / (p |d|) == |1 / d| pow2_recip(p) for p = 2^0 .. 2^15 and 30 M random d, all-ones mantissas included.
//
// usage: exactdiv_fuzz [seed]     prints one line per part and "OK"; exit code 1 and the first cases on a failure
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include "vk_exactdiv.hpp"

using namespace vk;

static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static float f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int failures = 0;
#define FAIL(...) do { if (failures++ < 20) { printf("FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

// the two floats that bracket 1 / b (equal when 1 / b is a float), nearer first
static void brackets(float b, float y[2]) {
    const double t = 1.0 / (double)b;
    const float n = (float)t;  // round to nearest
    float o = n;
    if ((double)n < t) o = nextafterf(n, INFINITY);
    else if ((double)n > t) o = nextafterf(n, -INFINITY);
    y[0] = n; y[1] = o;
}

static uint64_t seed_dependent = 0;
static void chain_case(float a, float b) {
    const float want = a / b;
    float y[2];
    brackets(b, y);
    for (int s = 0; s < 2; s++) {
        const float q = div_inrange_seeded(a, b, y[s]);
        const float q2 = div_by(a, recip_refine_seeded(b, y[s]));
        if (u_of(q) != u_of(q2)) FAIL("div_inrange and recip_refine + div_by disagree: a %a b %a", a, b);
        if (u_of(q) == u_of(want)) continue;
        if (s == 1 && (u_of(b) & 0x7fffffu) == 0x7fffffu) {  // the farther bracket, an all-ones divisor
            if (seed_dependent++ < 8) printf("  seed-dependent: %a / %a with seed %a (nearest %a): %a, IEEE %a\n", a, b, y[1], y[0], q, want);
            continue;
        }
        FAIL("chain: %a / %a seed %a (%s bracket) gives %a, IEEE %a", a, b, y[s], s ? "farther" : "nearer", q, want);
    }
}

static float random_inrange() {  // |f| in [2^-40, 2^40), either sign, any mantissa
    const uint64_t r = rnd();
    const uint32_t e = 127u - 40u + (uint32_t)((r >> 32) % 80u);
    return f_of(((uint32_t)(r >> 63) << 31) | (e << 23) | ((uint32_t)r & 0x7fffffu));
}

int main(int argc, char **argv) {
    if (argc > 1) rng_state = strtoull(argv[1], nullptr, 0) | 1ull;
    // ---- chain ----
    for (uint32_t m = 0; m < (1u << 23); m++) {
        const float b = f_of((127u << 23) | m);
        chain_case(1.0f, b);
        chain_case(random_inrange(), b);
    }
    for (uint32_t i = 0; i < 50000000u; i++) {
        float a = random_inrange(), b = random_inrange();
        if ((i & 15u) == 0u) b = f_of((u_of(b) & 0xff800000u) | ((i & 16u) ? 0x7fffffu : 0x7ffffeu));  // the top of a binade, often
        chain_case(a, b);
    }
    printf("chain: every mantissa x {1, random} and 50000000 random pairs, both bracketing seeds; %" PRIu64 " seed-dependent case(s) listed\n", seed_dependent);
    // ---- const ----
    uint64_t n_const = 0;
    for (uint32_t W = 1; W <= kDivConstMax; W++) {
        const float fw = (float)W, y = 1.0f / fw;
        for (uint32_t x = 0; x < W; x++, n_const++) {
            const float a = 2.0f * ((float)x + 0.5f);
            if (u_of(div_const(a, fw, y)) != u_of(a / fw)) FAIL("div_const: x %u W %u", x, W);
        }
    }
    printf("const: %" PRIu64 " cases\n", n_const);
    // ---- pow2 ----
    for (uint32_t i = 0; i < 30000000u; i++) {
        const uint64_t r = rnd();
        uint32_t m = (uint32_t)r & 0x7fffffu;
        if ((i & 63u) == 0u) m = 0x7fffffu;
        const uint32_t e = 127u - 81u + (uint32_t)((r >> 32) % 82u);  // |d| in [2^-81, 2)
        const float d = f_of(((uint32_t)(r >> 63) << 31) | (e << 23) | m);
        const float p = (float)(1u << ((r >> 40) & 15u));
        if (p * pow2_recip(p) != 1.0f) FAIL("pow2_recip(%a)", p);
        if (u_of(1.0f / (p * fabsf(d))) != u_of(fabsf(1.0f / d) * pow2_recip(p))) FAIL("pow2: d %a p %a", d, p);
    }
    printf("pow2: 30000000 cases\n");
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
