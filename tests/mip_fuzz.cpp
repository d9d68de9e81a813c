// TEST INFRASTRUCTURE: host build of the maximum-intensity projection's step and emptiness predicate (vokselis_amd/csrc/vk_tf.hpp:
// mip_update, mip_cell_empty) under ASan + UBSan.
// 1. Whenever vk::mip_cell_empty says a cell is empty, every f32 trilinear sample of that cell -- filtered as the march filters (x, then
//    y, then z, each lerp one fma) at fractions in [0, 1) including 0 and nextafterf(1, 0) -- leaves U with the bits it had under
//    vk::mip_update, for U = +0, the smallest subnormal, umax, values next to them and random U in [+0, umax].
// 2. A cell with a non-finite tap is never empty.
// 3. vk::mip_update (a select and a min) is the specification's fmaxf(U, tf_u(x)) + 0.0f, bit for bit, for every sample drawn -- of
//    empty and non-empty cells -- and every U of the list; its result is never -0 and stays in [+0, umax].
// Cells: u8 taps (0, 255, values around the window's lower end), f16 taps with subnormals, +-0, negatives, infinities, NaN; a sweep puts
// each of the 65 536 f16 patterns into a cell.  Windows: [0, 1], narrow ones whose lower end sits on or next to a data value, wide
// ones and ones wholly below or above the data.
// usage: mip_fuzz <cases> <seed>; prints "bad <n> of <cases> (<empty> empty, <nonfinite> non-finite)" and exits non-zero on any violation.
#include "vk_tf.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t state;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static float unit() { return (float)((rnd() >> 40) / 16777216.0); }  // [0, 1)

static float h2f(uint16_t h) {  // IEEE binary16 -> binary32, exact
    const uint32_t s = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31u, m = h & 1023u;
    float v;
    if (e == 0) v = ldexpf((float)m, -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = ldexpf((float)(m | 1024u), (int)e - 25);
    return s ? -v : v;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static long bad = 0, empty = 0, nonfinite = 0;

// one cell under one window: the three properties
static void check_cell(long c, const float t[8], int n, float k1, float k2) {
    const float umax = (float)(n - 1);
    bool finite = true;
    for (int b = 0; b < 8; b++) finite = finite && isfinite(t[b]);
    const bool is_empty = vk::mip_cell_empty(t, k1, k2, umax);
    if (!finite) {
        nonfinite++;
        if (is_empty) { if (bad < 10) printf("case %ld: a cell with a non-finite tap is empty\n", c); bad++; return; }
    }
    if (is_empty) empty++;
    const float Us[8] = {0.0f, 0x1p-149f, 0x1p-126f, unit() * umax, unit() * umax, nextafterf(umax, 0.0f), umax, unit() * 0x1p-20f};
    static const float fixed[4] = {0.0f, 0x1p-24f, 0.5f, 0.99999994f};  // 0.99999994 = nextafterf(1, 0)
    for (int s = 0; s < 48; s++) {
        const float fx = s < 16 ? fixed[s & 3] : unit(), fy = s < 16 ? fixed[(s >> 2) & 3] : unit(), fz = s < 16 ? fixed[(s + 1) & 3] : unit();
        const float c00 = fmaf(fx, t[1] - t[0], t[0]), c10 = fmaf(fx, t[3] - t[2], t[2]);
        const float c01 = fmaf(fx, t[5] - t[4], t[4]), c11 = fmaf(fx, t[7] - t[6], t[6]);
        const float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
        const float x = fmaf(fz, c1 - c0, c0);
        for (float U : Us) {
            const float got = vk::mip_update(U, x, k1, k2, umax);
            const float spec = fmaxf(U, vk::tf_u(x, k1, k2, umax)) + 0.0f;
            const bool ok = bits(got) == bits(spec) && !signbit(got) && got >= 0.0f && got <= umax && (!is_empty || bits(got) == bits(U));
            if (!ok) {
                if (bad < 10) printf("case %ld: n %d k1 %a k2 %a x %a U %a -> %a (specification %a, cell %s)\n", c, n, k1, k2, x, U, got, spec, is_empty ? "empty" : "not empty");
                bad++;
                return;
            }
        }
    }
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 20000;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    for (long c = 0; c < cases + 65536; c++) {
        const int n = (c & 1) ? 2 + (int)(rnd() % (vk::kTfMaxEntries - 1)) : (int[]){2, 3, 17, 256}[(c >> 1) & 3];
        const bool r8 = (c >> 3) & 1;
        // the window; for u8 its lower end is aimed at a data value v0 / 255 (on it, or a few ulps beside it)
        float lo, hi;
        const int v0 = (int)(rnd() % 256);
        const int dk = (int)(rnd() % 6);
        if (dk == 0) { lo = 0.0f; hi = 1.0f; }
        else if (dk == 1) { lo = (float)(v0 / 255.0); for (int q = (int)(rnd() % 5) - 2; q != 0; q += q < 0 ? 1 : -1) lo = nextafterf(lo, q < 0 ? -1.0f : 2.0f); hi = lo + 0x1p-10f + unit() * 0.7f; }
        else if (dk == 2) { lo = -2.0f + unit(); hi = 1.5f + 3.0f * unit(); }
        else if (dk == 3) { lo = unit() * 0.5f; hi = nextafterf(lo, 2.0f); for (int q = (int)(rnd() % 40); q > 0; q--) hi = nextafterf(hi, 2.0f); }
        else if (dk == 4) { lo = -9.0f; hi = -5.0f + unit(); }   // wholly below the data
        else { lo = 2.0f + unit(); hi = 70000.0f * (1.0f + unit()); }  // (mostly) above it
        float k1, k2;
        vk::tf_constants((uint32_t)n, lo, hi, r8, k1, k2);
        if (!(k1 > 0.0f) || !isfinite(k1) || !isfinite(k2)) continue;  // (windows so narrow that the constants overflow are not tested)
        float t[8];
        for (int b = 0; b < 8; b++) {
            if (r8) {
                int v = (int)(rnd() % 256);
                if (rnd() & 1) v = v0 + (int)(rnd() % 5) - 2;             // around the window's lower end
                if (rnd() % 3 == 0) v = (rnd() & 1) ? 255 : (int)(rnd() % 4);
                t[b] = (float)(v < 0 ? 0 : (v > 255 ? 255 : v));
            } else {
                uint16_t h = (uint16_t)rnd();
                const int hk = (int)(rnd() % 8);
                if (hk == 0) h = (uint16_t)(rnd() % 1024);                        // subnormals
                else if (hk == 1) h = (rnd() & 1) ? 0x8000 : 0x0000;               // +-0
                else if (hk == 2) h = (uint16_t)(0x8000 | (rnd() % 1024));         // negative subnormals
                else if (hk == 3) h = (uint16_t)(0x8000 | (rnd() % 0x3c00));        // negatives
                else if (hk == 4 && rnd() % 8 == 0) h = (uint16_t[]){0x7c00, 0xfc00, 0x7e01, 0xfc01}[rnd() % 4];  // +-inf / NaN (never empty)
                else if (hk == 5) h = (uint16_t)(0x2000 + rnd() % 0x1c00);          // 2^-7 .. 1
                else if (hk == 6) h = (uint16_t)(0x8000 | (0x2000 + rnd() % 0x1c00));
                t[b] = h2f(h);
            }
        }
        if (r8 && rnd() % 4 == 0) {  // the largest tap sits exactly on the value the window's lower end is aimed at
            for (int q = 0; q < 8; q++) t[q] = fminf(t[q], (float)v0);
            t[rnd() % 8] = (float)v0;
        }
        if (c >= cases) t[rnd() % 8] = h2f((uint16_t)(c - cases));  // the sweep: every f16 pattern as a tap
        check_cell(c, t, n, k1, k2);
    }
    printf("bad %ld of %ld (%ld empty, %ld non-finite)\n", bad, cases + 65536, empty, nonfinite);
    return bad ? 1 : 0;
}
