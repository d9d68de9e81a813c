// TEST INFRASTRUCTURE: host build of the shadows' shared header (vokselis_amd/csrc/vk_shadow.hpp) under ASan + UBSan, against brute force.
// 1. vk::shadow_desc accepts exactly the finite pairs with strength in [0, 1] and bias in [0, VK_SHADOW_MAX_BIAS = 1024]; a refused pair
//    leaves the descriptor untouched; an accepted one gives k = 1 - strength (one f32 rounding: the double difference rounded once) and
//    the bias itself, a -0 stored as +0.  The validation table of vk_set_shadows (every kind of refused value) is walked first.
// 2. vk::shadow_ts0 is the largest of the three candidates tb0, 0 and bias * dts (the product rounded once to f32), found here by
//    comparing all three; a NaN tb0 (a shadow ray along an axis from a point on a box plane) is ignored; the result is never negative
//    and never NaN for a finite bias * dts.
// 3. vk::shadow_k lies in [0, 1] for every strength the validation accepts, 1 at strength 0 and 0 at strength 1.
// usage: shadow_fuzz <cases> <seed>; prints "OK (<cases> cases)" or the first violations, and exits non-zero on any.
#include "vk_shadow.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t state;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static float unit() { return (float)((rnd() >> 40) / 16777216.0); }  // [0, 1)
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static long bad = 0;
static void fail(long c, const char *what, float a, float b) { if (bad < 10) printf("case %ld: %s (%a, %a)\n", c, what, a, b); bad++; }

// any f32: random bits half the time (NaNs, infinities, subnormals, huge values), values around the bounds otherwise
static float any_float(const float *edges, int n) {
    const uint64_t r = rnd();
    if (r & 1) return from_bits((uint32_t)(r >> 32));
    const float e = edges[(r >> 1) % (uint64_t)n];
    switch ((r >> 8) & 3) {
        case 0: return e;
        case 1: return nextafterf(e, INFINITY);
        case 2: return nextafterf(e, -INFINITY);
        default: return e + (unit() - 0.5f);
    }
}

static void check_desc(long c, float strength, float bias) {
    const bool ok = isfinite(strength) && isfinite(bias) && strength >= 0.0f && strength <= 1.0f && bias >= 0.0f && bias <= 1024.0f;
    vk::ShadowDesc D;
    D.k = -7.0f; D.bias = -9.0f;
    const char *why = vk::shadow_desc(strength, bias, D);
    if ((why == nullptr) != ok) return fail(c, ok ? "a valid pair is refused" : "an invalid pair is accepted", strength, bias);
    if (!ok) {
        if (D.k != -7.0f || D.bias != -9.0f) fail(c, "a refused pair changed the descriptor", strength, bias);
        return;
    }
    if (bits(D.k) != bits((float)(1.0 - (double)strength))) fail(c, "k is not 1 - strength rounded once", strength, D.k);
    if (!(D.k >= 0.0f && D.k <= 1.0f) || vk::shadow_k(strength) != D.k) fail(c, "k outside [0, 1]", strength, D.k);
    if (D.bias != bias || signbit(D.bias)) fail(c, "the bias is not stored as given (a -0 as +0)", bias, D.bias);
}

static void check_ts0(long c, float tb0, float bias, float dts) {
    const float prod = (float)((double)bias * (double)dts);  // one rounding (the double product of two floats is exact)
    const float got = vk::shadow_ts0(tb0, bias, dts);
    float want = 0.0f;  // the largest candidate, NaNs skipped
    if (tb0 == tb0 && tb0 > want) want = tb0;
    if (prod == prod && prod > want) want = prod;
    if (got != got || got != want || got < 0.0f) fail(c, "ts0 is not max(tb0, 0, bias * dts)", got, want);
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 400;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!state) state = 1;
    // the validation table: every kind of refused value, and the bounds themselves
    const float refused[][2] = {{NAN, 2.0f}, {0.5f, NAN}, {INFINITY, 2.0f}, {-INFINITY, 2.0f}, {0.5f, INFINITY}, {0.5f, -INFINITY}, {-0x1p-149f, 2.0f},
                                {nextafterf(1.0f, 2.0f), 2.0f}, {-1.0f, 2.0f}, {2.0f, 2.0f}, {0.5f, -0x1p-149f}, {0.5f, nextafterf(1024.0f, 2048.0f)},
                                {0.5f, -1.0f}, {0.5f, 1025.0f}, {NAN, NAN}};
    for (const auto &r : refused) {
        vk::ShadowDesc D{3.0f, 4.0f};
        if (vk::shadow_desc(r[0], r[1], D) == nullptr || D.k != 3.0f || D.bias != 4.0f) fail(-1, "the validation table: accepted, or the descriptor changed", r[0], r[1]);
    }
    const float accepted[][2] = {{0.0f, 0.0f}, {1.0f, 1024.0f}, {-0.0f, -0.0f}, {0x1p-149f, 0x1p-149f}, {0.7f, 2.0f}, {nextafterf(1.0f, 0.0f), nextafterf(1024.0f, 0.0f)}};
    for (const auto &a : accepted) check_desc(-2, a[0], a[1]);
    if (vk::shadow_k(0.0f) != 1.0f || vk::shadow_k(1.0f) != 0.0f) fail(-3, "k at the bounds", vk::shadow_k(0.0f), vk::shadow_k(1.0f));
    static const float s_edges[] = {0.0f, 1.0f, 0.5f, -0.0f}, b_edges[] = {0.0f, 1024.0f, 2.0f, 1.0f, -0.0f};
    static const float t_edges[] = {0.0f, -0.0f, 1.0f, 1.7320508f, -1.0f, 0x1p-20f, -0x1p-20f};
    for (long c = 0; c < cases; c++) {
        for (int j = 0; j < 256; j++) {
            check_desc(c, any_float(s_edges, 4), any_float(b_edges, 5));
            // ts0: tb0 anything (NaN, +-inf and -0 included), bias a valid one, dts a step of a volume of 1 .. 4096 voxels at dt_scale 2^-7 .. 4
            float bias = any_float(b_edges, 5);
            if (!(bias >= 0.0f && bias <= 1024.0f)) bias = 1024.0f * unit();
            const float dts = ldexpf(1.0f + unit(), (int)(rnd() % 6) - 7) / (float)(1 + rnd() % 4096);
            check_ts0(c, any_float(t_edges, 7), bias, dts);
        }
    }
    if (bad) {
        printf("bad %ld\n", bad);
        return 1;
    }
    printf("OK (%ld cases)\n", cases);
    return 0;
}
