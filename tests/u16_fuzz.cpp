// TEST INFRASTRUCTURE: host build of the emptiness predicates on R16_UNORM cells (vokselis_amd/csrc/vk_tf.hpp, vk_iso.hpp at SCALE_U16)
// under ASan + UBSan.  For random cells of u16 taps (0..65535, exact in f32), lerp weights in [0, 1) including 0 and nextafterf(1, 0),
// random tables, windows and thresholds -- every f32 trilinear sample filtered as the march filters (x, then y, then z, each lerp one fma):
// 1. table    a cell vk::tf_cell_empty calls empty: the looked-up alpha of every sample is +0, so the sample contributes exactly +0;
// 2. built-in a cell vk::builtin_cell_empty(t, SCALE_U16) calls empty: transfer_alpha<3> of every sample is +0;
// 3. MAX      a cell vk::mip_cell_empty calls empty: vk::mip_update leaves U = +0 as it was, bit for bit;
// 4. iso      a cell vk::iso_cell_empty calls empty: no sample is a hit under vk::iso_hit, with iso_k = vk::iso_k(iso, SCALE_U16).
// Exhaustively over all 65 536 tap values: transfer_alpha<3>(t) is +0 iff t <= 6553, iff vk::builtin_tap_empty(t, SCALE_U16); and
// vk::tf_constants / vk::iso_k at SCALE_U16 are the header's formulas (k1 = (n-1) / ((hi-lo) 65535) in double, iso * 65535.0f).
// usage: u16_fuzz <cases> <seed>; prints "bad <n> of <cases> (<e_tf> <e_builtin> <e_mip> <e_iso> empty)" and exits non-zero on any violation.
#include "vk_iso.hpp"
#include "vk_tf.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t state;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static float unit() { return (float)((rnd() >> 40) / 16777216.0); }  // [0, 1)
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool plus_zero(float a) { return bits(a) == 0u; }

// transfer_alpha<3> of vk_common.hpp (a device function there), restated: c = 0.9 * 65535, k1 = 1 / (65535 * 1.1), k2 = -0.1 / 1.1
static float transfer_alpha_u16(float x) {
    constexpr float k2 = (float)(-0.1 / 1.1), c = 58981.5f, k1 = (float)(1.0 / (65535.0 * 1.1));
    float s = fmaf(fminf(x, c), k1, k2);
    s = fminf(fmaxf(s, 0.0f), 1.0f);
    return (s * s) * fmaf(-2.0f, s, 3.0f);
}

static float filter(const float t[8], float fx, float fy, float fz) {
    const float c00 = fmaf(fx, t[1] - t[0], t[0]), c10 = fmaf(fx, t[3] - t[2], t[2]);
    const float c01 = fmaf(fx, t[5] - t[4], t[4]), c11 = fmaf(fx, t[7] - t[6], t[6]);
    const float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
    return fmaf(fz, c1 - c0, c0);
}

// the table lookup of the march (vk_march.hpp: tf_lookup), alpha only
static float tf_alpha(const float *rgba, int n, float x, float k1, float k2) {
    const float u = vk::tf_u(x, k1, k2, (float)(n - 1));
    const int i = vk::tf_index(u, n - 2);
    const float f = u - (float)i;
    return fmaf(f, rgba[4 * (i + 1) + 3] - rgba[4 * i + 3], rgba[4 * i + 3]);
}

static long bad = 0, e_tf = 0, e_bi = 0, e_mip = 0, e_iso = 0;
static void fail(long c, const char *what) { if (bad < 10) printf("case %ld: %s\n", c, what); bad++; }

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 20000;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    // ---- exhaustive: the built-in split at 6553 / 6554
    for (uint32_t v = 0; v < 65536u; v++) {
        const float t = (float)v;
        const bool zero = plus_zero(transfer_alpha_u16(t));
        if (zero != (v <= 6553u)) fail(-1, "transfer_alpha<3> is +0 on the wrong side of 6553");
        if (vk::builtin_tap_empty(t, vk::SCALE_U16) != (v <= 6553u)) fail(-1, "builtin_tap_empty(SCALE_U16) is not t <= 6553");
        const float u[8] = {t, t, t, t, t, t, t, t};
        if (vk::builtin_cell_empty(u, vk::SCALE_U16) != (v <= 6553u)) fail(-1, "builtin_cell_empty(SCALE_U16) of a uniform cell");
    }
    if (vk::iso_k(1.0f, vk::SCALE_U16) != 65535.0f || vk::iso_k(0.0f, vk::SCALE_U16) != 0.0f || vk::sample_scale(vk::SCALE_U16) != 65535.0) fail(-1, "the scale is not 65535");
    static const float fixed[4] = {0.0f, 0x1p-24f, 0.5f, 0x1.fffffep-1f};  // 0x1.fffffep-1 = nextafterf(1, 0)
    for (long c = 0; c < cases; c++) {
        // ---- a cell: taps anywhere, around one value, at the ends of the range, around the built-in threshold, 12-bit data
        float t[8];
        const uint32_t v0 = (uint32_t)(rnd() % 65536u);
        const int kind = (int)(rnd() % 6);
        for (int b = 0; b < 8; b++) {
            int64_t v = (int64_t)(rnd() % 65536u);
            if (kind == 1) v = (int64_t)v0 + (int64_t)(rnd() % 9) - 4;
            else if (kind == 2) v = (rnd() & 1) ? 65535 - (int64_t)(rnd() % 3) : (int64_t)(rnd() % 3);
            else if (kind == 3) v = 6553 + (int64_t)(rnd() % 5) - 3 - ((rnd() % 4 == 0) ? (int64_t)(rnd() % 6000) : 0);
            else if (kind == 4) v = (int64_t)(rnd() % 4096u);
            else if (kind == 5) v = (int64_t)v0 + (int64_t)(rnd() % 2001) - 1000;
            t[b] = (float)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
        }
        float m = t[0], M = t[0];
        for (int b = 1; b < 8; b++) { m = fminf(m, t[b]); M = fmaxf(M, t[b]); }
        // ---- a table (runs of alpha +0 and -0) over a window in sample values, through tf_constants at SCALE_U16
        const int n = (int[]){2, 3, 17, 64, 256}[rnd() % 5];
        float rgba[4 * 256];
        for (int j = 0; j < n; j++) {
            for (int k = 0; k < 3; k++) rgba[4 * j + k] = unit();
            rgba[4 * j + 3] = rnd() % 3 ? unit() * 0.4f : ((rnd() & 1) ? 0.0f : -0.0f);
        }
        { const int a = (int)(rnd() % n), len = 1 + (int)(rnd() % (n / 2 + 1)); for (int j = a; j < n && j < a + len; j++) rgba[4 * j + 3] = 0.0f; }
        float lo, hi;
        const int wk = (int)(rnd() % 4);
        if (wk == 0) { lo = 0.0f; hi = 1.0f; }
        else if (wk == 1) { lo = (m - 50.0f * unit()) / 65535.0f; hi = (M + 1.0f + 50.0f * unit()) / 65535.0f; }  // around the cell
        else if (wk == 2) { lo = unit() * 0.05f; hi = lo + 4095.0f / 65535.0f * (0.1f + unit()); }                  // a 12-bit window
        else { lo = 4.0f * unit() - 2.0f; hi = lo + 0.001f + 3.0f * unit(); }
        float k1, k2;
        vk::tf_constants((uint32_t)n, lo, hi, vk::SCALE_U16, k1, k2);
        {
            const double span = (double)hi - (double)lo, nm1 = (double)n - 1.0;
            if (bits(k1) != bits((float)(nm1 / (span * 65535.0))) || bits(k2) != bits((float)(-(double)lo * nm1 / span))) fail(c, "tf_constants(SCALE_U16)");
        }
        uint32_t prefix[257];
        vk::tf_alpha_prefix(rgba, (uint32_t)n, prefix);
        const float umax = (float)(n - 1);
        const float iso = wk == 0 ? (M + (float)((int)(rnd() % 5) - 2)) / 65535.0f : (rnd() & 1 ? (M + 1.0f) / 65535.0f : unit());
        const float ik = vk::iso_k(iso, vk::SCALE_U16);
        if (bits(ik) != bits(iso * 65535.0f)) fail(c, "iso_k(SCALE_U16)");
        const bool tf_e = vk::tf_cell_empty(t, prefix, n, k1, k2), bi_e = vk::builtin_cell_empty(t, vk::SCALE_U16);
        const bool mip_e = vk::mip_cell_empty(t, k1, k2, umax), iso_e = vk::iso_cell_empty(t, ik);
        e_tf += tf_e; e_bi += bi_e; e_mip += mip_e; e_iso += iso_e;
        { bool all = true; for (int b = 0; b < 8; b++) all = all && t[b] <= 6553.0f; if (bi_e != all) fail(c, "builtin_cell_empty(SCALE_U16) is not: every tap <= 6553"); }
        if (iso_e != (M < ik)) fail(c, "iso_cell_empty is not M < iso_k on finite taps");
        for (int s = 0; s < 40; s++) {
            const float fx = s < 16 ? fixed[s & 3] : unit(), fy = s < 16 ? fixed[(s >> 2) & 3] : unit(), fz = s < 16 ? fixed[(s + 1) & 3] : unit();
            const float x = filter(t, fx, fy, fz);
            if (!(x >= m && x <= M)) { fail(c, "a sample left [m, M]"); break; }
            if (tf_e) {
                const float a = tf_alpha(rgba, n, x, k1, k2), A = unit();
                const float w = (1.0f - A) * a;
                if (!plus_zero(a) || !plus_zero(w)) { fail(c, "table: a sample of an empty cell has alpha != +0"); break; }
                const float G = unit() * 3.0f - 1.0f;
                if (bits(fmaf(w, rgba[0] * 1e30f, G)) != bits(G) || bits(A + w) != bits(A)) { fail(c, "table: an empty sample moved an accumulator"); break; }
            }
            if (bi_e && !plus_zero(transfer_alpha_u16(x))) { fail(c, "built-in: a sample of an empty cell has alpha != +0"); break; }
            if (mip_e && bits(vk::mip_update(0.0f, x, k1, k2, umax)) != 0u) { fail(c, "MAX: a sample of an empty cell raised U"); break; }
            if (iso_e && vk::iso_hit(x, ik)) { fail(c, "iso: a sample of an empty cell hits"); break; }
        }
    }
    printf("bad %ld of %ld (%ld %ld %ld %ld empty)\n", bad, cases, e_tf, e_bi, e_mip, e_iso);
    return bad ? 1 : 0;
}
