// TEST INFRASTRUCTURE: host build of the isosurface's shared header (vokselis_amd/csrc/vk_iso.hpp) under ASan + UBSan.
// 1. Whenever vk::iso_cell_empty says a cell is empty, no f32 trilinear sample of that cell -- filtered as the march filters (x, then y,
//    then z, each lerp one fma) at fractions in [0, 1) including 0 and nextafterf(1, 0) -- is a hit under vk::iso_hit.
// 2. A cell with a non-finite tap is never empty; a +inf sample is a hit, a NaN sample is none.
// 3. vk::iso_desc accepts exactly the finite thresholds, the colours within +-VK_TF_MAX_COLOUR and refine <= VK_ISO_MAX_REFINE, and
//    leaves the descriptor it rejects untouched in iso_k; vk::iso_k is iso * 255.0f rounded once for R8 and iso itself for R16F.
// 4. vk::iso_refine returns the a of a literal enumeration of the specification's loop (m = a + 2^-i, written with ldexpf), for
//    monotone and for arbitrary hit functions, at every depth 0 .. 16; a is a dyadic of R bits in [0, 1 - 2^-R].
// 5. A ray's "no sample yet" value, NaN, meets no threshold, -inf and +inf included (a -inf would meet iso_k = -inf).
// Cells: u8 taps around the threshold, f16 taps with subnormals, +-0, negatives, infinities, NaN; a sweep puts each of the 65 536 f16
// patterns into a cell.  Thresholds: on a tap, next to a tap, between taps, below and above all of them.
// usage: iso_fuzz <cases> <seed>; prints "bad <n> of <cases> (<empty> empty, <nonfinite> non-finite)" and exits non-zero on any violation.
#include "vk_iso.hpp"

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
static void fail(long c, const char *what) { if (bad < 10) printf("case %ld: %s\n", c, what); bad++; }

// one cell under one threshold: properties 1 and 2
static void check_cell(long c, const float t[8], float k) {
    bool finite = true;
    for (int b = 0; b < 8; b++) finite = finite && isfinite(t[b]);
    const bool is_empty = vk::iso_cell_empty(t, k);
    if (!finite) {
        nonfinite++;
        if (is_empty) return fail(c, "a cell with a non-finite tap is empty");
    }
    if (is_empty) empty++;
    static const float fixed[4] = {0.0f, 0x1p-24f, 0.5f, 0.99999994f};  // 0.99999994 = nextafterf(1, 0)
    for (int s = 0; s < 48; s++) {
        const float fx = s < 16 ? fixed[s & 3] : unit(), fy = s < 16 ? fixed[(s >> 2) & 3] : unit(), fz = s < 16 ? fixed[(s + 1) & 3] : unit();
        const float c00 = fmaf(fx, t[1] - t[0], t[0]), c10 = fmaf(fx, t[3] - t[2], t[2]);
        const float c01 = fmaf(fx, t[5] - t[4], t[4]), c11 = fmaf(fx, t[7] - t[6], t[6]);
        const float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
        const float x = fmaf(fz, c1 - c0, c0);
        if (is_empty && vk::iso_hit(x, k)) {
            if (bad < 10) printf("case %ld: k %a: sample %a of an empty cell hits\n", c, k, x);
            bad++;
            return;
        }
        if (vk::iso_hit(x, k) != (x >= k)) return fail(c, "iso_hit is not x >= k");
    }
    if (vk::iso_hit(NAN, k) || !vk::iso_hit(INFINITY, k) || vk::iso_hit(-INFINITY, k) != (k == -INFINITY)) return fail(c, "iso_hit on NaN / +inf / -inf");
    if (vk::iso_hit(NAN, -INFINITY) || vk::iso_hit(NAN, INFINITY)) return fail(c, "NaN meets an infinite threshold");
}

// property 3
static void check_validation(long c) {
    const float specials[] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, 1.0f, -3.5f, 3.0e38f, 1e30f, -1e30f, nextafterf(1e30f, INFINITY), nextafterf(-1e30f, -INFINITY), 0x1p-149f};
    const int ns = (int)(sizeof specials / sizeof specials[0]);
    auto pick = [&]() { return rnd() % 3 ? (unit() - 0.5f) * 4.0f : specials[rnd() % ns]; };
    const float iso = pick();
    const float rgb[3] = {pick(), pick(), pick()};
    const uint32_t refine = rnd() % 4 ? (uint32_t)(rnd() % 17) : (uint32_t)(17 + rnd() % 5 + ((rnd() & 1) ? 0xfffffff0u : 0u));
    const bool r8 = rnd() & 1;
    vk::IsoDesc D{};
    D.iso_k = -123.0f;
    const char *msg = vk::iso_desc(iso, rgb, refine, r8, D);
    bool want = isfinite(iso) && refine <= 16u;
    for (int k = 0; k < 3; k++) want = want && isfinite(rgb[k]) && fabsf(rgb[k]) <= 1e30f;
    if ((msg == nullptr) != want) return fail(c, "iso_desc accepts / rejects the wrong set");
    if (msg) { if (D.iso_k != -123.0f) fail(c, "a rejected descriptor was written"); return; }
    const float k = r8 ? iso * 255.0f : iso;
    if (bits(D.iso_k) != bits(k) || bits(vk::iso_k(iso, r8)) != bits(k)) return fail(c, "iso_k");
    if (bits(D.r) != bits(rgb[0]) || bits(D.g) != bits(rgb[1]) || bits(D.b) != bits(rgb[2]) || D.refine != refine) return fail(c, "iso_desc fields");
    if (vk::iso_k(1.0f, true) != 255.0f || vk::iso_k(0.0f, true) != 0.0f) return fail(c, "iso_k(1.0) != 255");
}

// property 4
static void check_refine(long c) {
    const uint32_t R = (uint32_t)(rnd() % 17);
    const bool monotone = rnd() & 1;
    const float cross = unit();  // monotone: the samples from `cross` steps back onwards are below the threshold
    const uint64_t pattern = rnd();
    uint32_t calls = 0;
    auto hits = [&](float m) { calls++; return monotone ? m <= cross : (bool)((pattern >> (bits(m) % 61u)) & 1u); };
    const float got = vk::iso_refine(R, hits);
    float a = 0.0f;
    for (uint32_t i = 1; i <= R; i++) {
        const float m = a + ldexpf(1.0f, -(int)i);
        if (hits(m)) a = m;
    }
    const float top = 1.0f - ldexpf(1.0f, -(int)R);
    if (bits(got) != bits(a) || calls != 2 * R || !(got >= 0.0f && got <= top) || ldexpf(got, (int)R) != floorf(ldexpf(got, (int)R)))
        return fail(c, "iso_refine parts from the enumeration");
    if (monotone && R > 0 && !(got <= cross && cross - got < ldexpf(1.0f, -(int)R) + 0x1p-24f)) return fail(c, "iso_refine misses a monotone crossing");
    // the position: fma(-m, s, p), and a = 0 gives p's value
    const float s = (unit() - 0.5f) * 0.1f, p = unit();
    if (bits(vk::iso_back(got, s, p)) != bits(fmaf(-got, s, p)) || vk::iso_back(0.0f, s, p) != p) return fail(c, "iso_back");
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 20000;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    for (long c = 0; c < cases + 65536; c++) {
        const bool r8 = (c >> 3) & 1;
        float t[8];
        const int v0 = (int)(rnd() % 256);
        for (int b = 0; b < 8; b++) {
            if (r8) {
                int v = (int)(rnd() % 256);
                if (rnd() & 1) v = v0 + (int)(rnd() % 5) - 2;  // around the threshold's value
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
        if (c >= cases) t[rnd() % 8] = h2f((uint16_t)(c - cases));  // the sweep: every f16 pattern as a tap
        float M = -INFINITY;
        for (int b = 0; b < 8; b++) if (isfinite(t[b])) M = fmaxf(M, t[b]);
        if (!isfinite(M)) M = 0.0f;
        // the threshold: on the largest tap, one ulp beside it, through iso_k from a public value, or anywhere
        float k;
        const int kk = (int)(rnd() % 6);
        if (kk == 0) k = M;
        else if (kk == 1) k = nextafterf(M, INFINITY);
        else if (kk == 2) k = nextafterf(M, -INFINITY);
        else if (kk == 3) k = vk::iso_k(r8 ? (float)(v0 / 255.0) : M * (0.5f + unit()), r8);
        else if (kk == 4) k = r8 ? 300.0f * unit() - 20.0f : 4.0f * unit() - 2.0f;
        else if (rnd() % 4) k = (rnd() & 1) ? -70000.0f : 70000.0f;
        else k = vk::iso_k((rnd() & 1) ? -3.0e38f : 3.0e38f, true);  // a finite public value whose R8 threshold overflows: -inf / +inf
        check_cell(c, t, k);
        if (c % 4 == 0) check_validation(c);
        if (c % 4 == 1) check_refine(c);
    }
    printf("bad %ld of %ld (%ld empty, %ld non-finite)\n", bad, cases + 65536, empty, nonfinite);
    return bad ? 1 : 0;
}
