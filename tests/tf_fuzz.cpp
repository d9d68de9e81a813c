// TEST INFRASTRUCTURE: host build of the runtime transfer function's emptiness predicate (vokselis_amd/csrc/vk_tf.hpp) under ASan + UBSan.
// Whenever vk::tf_cell_empty says a cell is empty, every f32 trilinear sample of that cell -- filtered as the march filters (x, then y,
// then z, each lerp one fma) at fractions in [0, 1) including 0 and nextafterf(1, 0) -- must look up alpha == +0 in the table.
// Tables: sparse alphas, a single non-zero entry, every entry non-zero.  Domains inside and beyond the data range.  Cells: u8 taps, and
// f16 taps with subnormals, +-0, negatives, infinities, NaN and values on the guard boundaries of the table.
// usage: tf_fuzz <cases> <seed>; prints "bad <n> of <cases> (<empty> empty)" and exits non-zero on any violation.
//        tf_fuzz constants <n> <lo> <hi> <r8>: prints vk::tf_constants' k1 and k2 (hex floats) for the host restatement to be held to.
#include "vk_tf.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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
static uint16_t f2h_trunc(float f) {  // some binary16 near f (only used to aim taps at a value)
    for (uint16_t h = 0;; h++) { if (h2f(h) >= f || h == 0x7bff) return h; }
}

// a table entry's alpha, looked up as the kernel does (vk_march.hpp: tf_lookup)
static float lookup_alpha(const std::vector<float> &T, int n, float x, float k1, float k2) {
    const float u = vk::tf_u(x, k1, k2, (float)(n - 1));
    const int i = vk::tf_index(u, n - 2);
    const float f = u - (float)i;
    return fmaf(f, T[4 * (i + 1) + 3] - T[4 * i + 3], T[4 * i + 3]);
}

int main(int argc, char **argv) {
    if (argc == 6 && strcmp(argv[1], "constants") == 0) {
        float k1, k2;
        vk::tf_constants((uint32_t)atoi(argv[2]), strtof(argv[3], nullptr), strtof(argv[4], nullptr), atoi(argv[5]) != 0, k1, k2);
        printf("%a %a\n", (double)k1, (double)k2);
        return 0;
    }
    const long cases = argc > 1 ? atol(argv[1]) : 20000;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    long bad = 0, empty = 0;
    for (long c = 0; c < cases; c++) {
        const int n = 2 + (int)(rnd() % (vk::kTfMaxEntries - 1));
        std::vector<float> T(4 * (size_t)n, 0.0f);
        const int kind = (int)(c % 3);
        for (int j = 0; j < n; j++) {
            for (int k = 0; k < 3; k++) T[4 * j + k] = unit() * 2.0f - 0.5f;
            float a = 0.0f;
            if (kind == 0) a = (rnd() % 5 == 0) ? unit() : ((rnd() & 1) ? -0.0f : 0.0f);  // sparse (and signed zeros)
            else if (kind == 2) a = 0x1p-20f + unit() * 0.9f;                                // every entry non-zero
            T[4 * j + 3] = a;
        }
        if (kind == 1) T[4 * (rnd() % n) + 3] = 0x1p-30f + unit();  // a single non-zero entry
        std::vector<uint32_t> prefix(n + 1);
        vk::tf_alpha_prefix(T.data(), (uint32_t)n, prefix.data());
        const bool r8 = (c >> 2) & 1;
        // domains inside and beyond the data range ([0, 1] for u8; f16 values around it), narrow ones too
        float lo, hi;
        const int dk = (int)(rnd() % 4);
        if (dk == 0) { lo = 0.0f; hi = 1.0f; }
        else if (dk == 1) { lo = unit() * 0.8f; hi = lo + 0x1p-10f + unit() * 0.3f; }
        else if (dk == 2) { lo = -2.0f + unit(); hi = 1.5f + 3.0f * unit(); }
        else { lo = unit() * 0.5f; hi = nextafterf(lo, 2.0f) ; for (int q = (int)(rnd() % 40); q > 0; q--) hi = nextafterf(hi, 2.0f); }
        float k1, k2;
        vk::tf_constants((uint32_t)n, lo, hi, r8, k1, k2);
        if (!(k1 > 0.0f) || !isfinite(k1) || !isfinite(k2)) continue;  // (domains so narrow that the constants overflow are not tested)
        float t[8];
        // taps aimed at the guard boundaries: values whose u sits on or next to an entry boundary
        const float target = lo + (hi - lo) * (float)(rnd() % n) / (float)(n - 1);
        for (int b = 0; b < 8; b++) {
            if (r8) {
                int v = (int)(rnd() % 256);
                if (rnd() & 1) v = (int)lrintf(target * 255.0f) + (int)(rnd() % 5) - 2;
                if (rnd() % 3 == 0) v = (int)(rnd() % 4);
                t[b] = (float)(v < 0 ? 0 : (v > 255 ? 255 : v));
            } else {
                uint16_t h = (uint16_t)rnd();
                const int hk = (int)(rnd() % 8);
                if (hk == 0) h = (uint16_t)(rnd() % 1024);                        // subnormals
                else if (hk == 1) h = (rnd() & 1) ? 0x8000 : 0x0000;               // +-0
                else if (hk == 2) h = f2h_trunc(fabsf(target)) + (uint16_t)(rnd() % 3) - 1 + ((target < 0.0f) ? 0x8000 : 0);
                else if (hk == 3) h = (uint16_t)(0x8000 | (rnd() % 0x3c00));        // negatives
                else if (hk == 4 && rnd() % 16 == 0) h = (rnd() & 1) ? 0x7c00 : 0x7e01;  // inf / NaN (never empty)
                else if (hk == 5) h = (uint16_t)(0x2000 + rnd() % 0x1c00);          // 2^-7 .. 1
                t[b] = h2f(h);
            }
        }
        if (!vk::tf_cell_empty(t, prefix.data(), n, k1, k2)) continue;
        empty++;
        static const float fixed[4] = {0.0f, 0x1p-24f, 0.5f, 0.99999994f};  // 0.99999994 = nextafterf(1, 0)
        for (int s = 0; s < 64; s++) {
            const float fx = s < 16 ? fixed[s & 3] : unit(), fy = s < 16 ? fixed[(s >> 2) & 3] : unit(), fz = s < 16 ? fixed[(s + 1) & 3] : unit();
            const float c00 = fmaf(fx, t[1] - t[0], t[0]), c10 = fmaf(fx, t[3] - t[2], t[2]);
            const float c01 = fmaf(fx, t[5] - t[4], t[4]), c11 = fmaf(fx, t[7] - t[6], t[6]);
            const float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
            const float x = fmaf(fz, c1 - c0, c0);
            const float a = lookup_alpha(T, n, x, k1, k2);
            if (!(a == 0.0f && !signbit(a))) {
                if (bad < 10) printf("case %ld: n %d domain [%a, %a] x %a alpha %a\n", c, n, lo, hi, x, a);
                bad++;
                break;
            }
        }
    }
    printf("bad %ld of %ld (%ld empty)\n", bad, cases, empty);
    return bad ? 1 : 0;
}
