// TEST INFRASTRUCTURE: host build of the lone-speckle code of the built-in skip maps (vokselis_amd/csrc/vk_tf.hpp: vk::speckle_code, the
// encoder of pack_cells_kernel and cell_occ_kernel, and vk::speckle_proven, the decoder of march()) under ASan + UBSan.  Whenever the
// decoder calls a sample proven, the f32 filter chain of both u8 cell layouts -- x, then y, then z, each lerp one fma; PACKED takes the
// x-differences of its taps, PACKED_PAIRS reads them as stored f16 deltas -- followed by transfer_alpha<1> must give alpha == +0.
// Cells: every hot value 26..255 against every cold maximum 0..25 in all eight corners, the other cold taps drawn at or below the
// maximum.  Weights: 0, the largest float below 1, a few ulp either side of every q/16 and of its square and cube roots (spent on one,
// two or three axes, the rest at the largest float below 1), and random ones.
// The encoder is held to an integer restatement on every such cell, and returns 0 for cells with no hot tap, with two or more, with
// q = 0 and with a tap that is no u8 value.
// usage: speckle_fuzz <random weights per cell> <seed>; prints "bad <n> of <samples> (<proven> proven); stand-in range <p> of <n> proven"
// and exits non-zero on any violation.
#include "vk_tf.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

static uint64_t state;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static float unit() { return (float)((rnd() >> 40) / 16777216.0); }  // [0, 1)

// transfer_alpha<1> of vk_common.hpp (a device function there), restated: filtered u8 taps on their 0..255 scale
static float transfer_alpha_u8(float x) {
    constexpr float k2 = (float)(-0.1 / 1.1), c = 229.5f, k1 = (float)(1.0 / (255.0 * 1.1));
    float s = fmaf(fminf(x, c), k1, k2);
    s = fminf(fmaxf(s, 0.0f), 1.0f);
    return (s * s) * fmaf(-2.0f, s, 3.0f);
}

// PACKED (P8): the x-differences of the taps, computed
static float filter_p8(const float t[8], float fx, float fy, float fz) {
    const float c00 = fmaf(fx, t[1] - t[0], t[0]), c10 = fmaf(fx, t[3] - t[2], t[2]);
    const float c01 = fmaf(fx, t[5] - t[4], t[4]), c11 = fmaf(fx, t[7] - t[6], t[6]);
    const float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
    return fmaf(fz, c1 - c0, c0);
}

// PACKED_PAIRS (P16): (tap, delta) pairs of f16, as pack_cells_kernel stores them; an f16 holds every integer up to 2048 exactly
static float f16_exact(float v) {
    if (!(fabsf(v) <= 2048.0f && v == rintf(v))) { printf("not exact in f16: %a\n", v); exit(2); }
    return v;
}
static float filter_p16(const float t[8], float fx, float fy, float fz) {
    float tap[4], delta[4];
    for (int k = 0; k < 4; k++) { tap[k] = f16_exact(t[2 * k]); delta[k] = f16_exact(t[2 * k + 1] - t[2 * k]); }
    const float c00 = fmaf(fx, delta[0], tap[0]), c10 = fmaf(fx, delta[1], tap[1]);
    const float c01 = fmaf(fx, delta[2], tap[2]), c11 = fmaf(fx, delta[3], tap[3]);
    const float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
    return fmaf(fz, c1 - c0, c0);
}

static bool plus_zero(float a) { return a == 0.0f && !signbit(a); }

static long bad = 0, samples = 0, proven = 0;

static void fail(const char *what, const float t[8], float fx, float fy, float fz, uint32_t code, float a8, float a16) {
    if (bad < 10)
        printf("%s: taps %g %g %g %g %g %g %g %g code 0x%02x at (%a, %a, %a): alpha %a / %a\n", what, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7],
               code, fx, fy, fz, a8, a16);
    bad++;
}

// one sample of a coded cell: proven implies alpha +0 on both chains
static bool sample(const float t[8], uint32_t code, float fx, float fy, float fz) {
    samples++;
    if (!vk::speckle_proven(code, fx, fy, fz)) return false;
    proven++;
    const float a8 = transfer_alpha_u8(filter_p8(t, fx, fy, fz)), a16 = transfer_alpha_u8(filter_p16(t, fx, fy, fz));
    if (!plus_zero(a8) || !plus_zero(a16)) fail("proven sample with alpha != +0", t, fx, fy, fz, code, a8, a16);
    return true;
}

static float step_ulps(float x, int n) {
    for (; n > 0; n--) x = nextafterf(x, 2.0f);
    for (; n < 0; n++) x = nextafterf(x, -1.0f);
    return x;
}

// the fraction that gives weight w toward the corner's side of an axis: f itself on the upper side, 1 - f on the lower (clamped into [0, 1))
static float frac_for(float w, bool upper) {
    const float f = upper ? w : 1.0f - w;
    return fminf(fmaxf(f, 0.0f), 0x1.fffffep-1f);
}

static void adversarial(const float t[8], uint32_t code) {
    const bool ux = code & 0x10u, uy = code & 0x20u, uz = code & 0x40u;
    static const float ones[2] = {0x1.fffffep-1f, 1.0f};
    float ws[2 + 15 * 3 * 5];
    int n = 0;
    ws[n++] = 0.0f;
    ws[n++] = 0x1.fffffep-1f;
    for (int q = 1; q <= 15; q++) {
        const float lim = (float)q / 16.0f;
        for (int u = -2; u <= 2; u++) { ws[n++] = step_ulps(lim, u); ws[n++] = step_ulps(sqrtf(lim), u); ws[n++] = step_ulps(cbrtf(lim), u); }
    }
    for (int i = 0; i < n; i++) {
        const float w = ws[i];
        for (int o = 0; o < 2; o++) {
            const float one = ones[o];
            sample(t, code, frac_for(w, ux), frac_for(one, uy), frac_for(one, uz));  // the whole weight on one axis
            sample(t, code, frac_for(one, ux), frac_for(w, uy), frac_for(one, uz));
            sample(t, code, frac_for(one, ux), frac_for(one, uy), frac_for(w, uz));
            sample(t, code, frac_for(w, ux), frac_for(w, uy), frac_for(one, uz));    // on two (the square roots meet the limit)
            sample(t, code, frac_for(one, ux), frac_for(w, uy), frac_for(w, uz));
            sample(t, code, frac_for(w, ux), frac_for(one, uy), frac_for(w, uz));
        }
        sample(t, code, frac_for(w, ux), frac_for(w, uy), frac_for(w, uz));          // on three (the cube roots)
    }
}

static void expect_code(const float t[8], uint32_t want, const char *what) {
    const uint32_t got = vk::speckle_code(t);
    if (got != want) {
        if (bad < 10) printf("%s: taps %g %g %g %g %g %g %g %g: code 0x%02x, expected 0x%02x\n", what, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], got, want);
        bad++;
    }
}

int main(int argc, char **argv) {
    const long per_cell = argc > 1 ? atol(argv[1]) : 64;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    float t[8];
    long coded_cells = 0;
    for (int v = 26; v <= 255; v++)
        for (int m = 0; m <= 25; m++)
            for (int corner = 0; corner < 8; corner++) {
                // cold taps: one of them is the maximum, the others the maximum, 0 or drawn at or below it
                const int fill = (int)(rnd() % 3);
                for (int b = 0; b < 8; b++) t[b] = (float)(fill == 0 ? m : (fill == 1 ? 0 : (int)(rnd() % (uint64_t)(m + 1))));
                int at = (int)(rnd() % 7);
                if (at >= corner) at++;
                t[at] = (float)m;
                t[corner] = (float)v;
                const int q = (16 * (25 - m)) / (v - m);  // the encoder's limit in integers
                const uint32_t want = q >= 1 ? (0x80u | ((uint32_t)corner << 4) | (uint32_t)q) : 0u;
                if (q > 15) { printf("q = %d\n", q); return 2; }
                expect_code(t, want, q >= 1 ? "single hot tap" : "q = 0");
                if (!want) continue;
                coded_cells++;
                adversarial(t, want);
                for (long s = 0; s < per_cell; s++) sample(t, want, unit(), unit(), unit());
                // a second hot tap, and none: never coded
                float u[8];
                for (int b = 0; b < 8; b++) u[b] = t[b];
                u[at] = (float)(26 + (int)(rnd() % 230));
                expect_code(u, 0u, "two hot taps");
                u[at] = (float)m; u[corner] = (float)m;
                expect_code(u, 0u, "no hot tap");
                u[corner] = (float)v; u[at] = rnd() % 2 ? NAN : (rnd() % 2 ? -1.0f : 256.0f);
                expect_code(u, 0u, "a tap that is no u8 value");
            }
    for (int k = 0; k < 8; k++) {  // all taps hot
        for (int b = 0; b < 8; b++) t[b] = 255.0f;
        expect_code(t, 0u, "all hot");
        for (int b = 0; b < 8; b++) t[b] = b <= k ? 26.0f : 0.0f;
        if (k >= 1) expect_code(t, 0u, "several hot taps");
    }
    // non-vacuity: the stand-in's range (hot 26..41, cold 0..20, uniform weights); the bound alone proves about 85 % of these
    long sp = 0, sn = 0;
    for (long c = 0; c < 20000; c++) {
        for (int b = 0; b < 8; b++) t[b] = (float)(rnd() % 21);
        const int corner = (int)(rnd() % 8);
        t[corner] = (float)(26 + (int)(rnd() % 16));
        const uint32_t code = vk::speckle_code(t);
        sn++;
        if (code && sample(t, code, unit(), unit(), unit())) sp++;
    }
    printf("bad %ld of %ld (%ld proven, %ld coded cells); stand-in range %ld of %ld proven\n", bad, samples, proven, coded_cells, sp, sn);
    if (sp * 4 < sn) { printf("the stand-in range proves fewer than a quarter: the path is not exercised\n"); return 1; }
    return bad ? 1 : 0;
}
