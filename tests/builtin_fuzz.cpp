// TEST INFRASTRUCTURE: host build of the built-in transfer's emptiness predicate (vokselis_amd/csrc/vk_tf.hpp: vk::builtin_cell_empty, the
// predicate of pack_cells_kernel and cell_occ_kernel) under ASan + UBSan.  Whenever it says a cell is empty, every f32 trilinear sample of
// that cell -- filtered as the march filters (x, then y, then z, each lerp one fma) at fractions in [0, 1) including 0 and
// nextafterf(1, 0) -- must have transfer_alpha == +0 at the cell's scale: f16 taps as values (SCALE 0); u8 taps on 0..255 (SCALE 1) and
// the same times 2^-24 (SCALE 2, the staged kernel's u8 taps).
// Cells: random cells of edge values; every one of the 65 536 f16 patterns as a uniform cell and next to a 0 tap; every u8 value the same.
// usage: builtin_fuzz <cases> <seed>; prints "bad <n> of <cells> (<empty> empty)" and exits non-zero on any violation.
//        builtin_fuzz taps: prints the predicate of every tap alone, '1' empty / '0' not: 65 536 f16 patterns in order, a newline, the
//        256 u8 values (for the numpy restatement to be held to).
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

// transfer_alpha of vk_common.hpp (a device function there), restated: min(x, c), then smoothstep's affine map as one fma whose constants
// carry the scale of x, then t*t*(3 - 2t)
template <int SCALE>
static float transfer_alpha(float x) {
    constexpr float k2 = (float)(-0.1 / 1.1);
    constexpr float c = SCALE == 0 ? 0.9f : (SCALE == 1 ? 229.5f : 229.5f * 0x1p-24f);
    constexpr float k1 = SCALE == 0 ? (float)(1.0 / 1.1) : (SCALE == 1 ? (float)(1.0 / (255.0 * 1.1)) : (float)(1.0 / (255.0 * 1.1)) * 16777216.0f);
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

static bool plus_zero(float a) { return a == 0.0f && !signbit(a); }

static long bad = 0, empty = 0, cells = 0;

// one cell: if the predicate calls it empty, 64 samples at fixed and random fractions must have alpha +0 at every scale of its format
static void check(const float t[8], bool f16, const char *what) {
    cells++;
    if (!vk::builtin_cell_empty(t, f16)) return;
    empty++;
    static const float fixed[4] = {0.0f, 0x1p-24f, 0.5f, 0x1.fffffep-1f};  // 0x1.fffffep-1 = nextafterf(1, 0)
    float t24[8];
    for (int b = 0; b < 8; b++) t24[b] = t[b] * 0x1p-24f;  // (exact: u8 values)
    for (int s = 0; s < 64; s++) {
        const float fx = s < 16 ? fixed[s & 3] : unit(), fy = s < 16 ? fixed[(s >> 2) & 3] : unit(), fz = s < 16 ? fixed[(s + 1) & 3] : unit();
        float a[2];
        if (f16) a[0] = a[1] = transfer_alpha<0>(filter(t, fx, fy, fz));
        else { a[0] = transfer_alpha<1>(filter(t, fx, fy, fz)); a[1] = transfer_alpha<2>(filter(t24, fx, fy, fz)); }
        if (!plus_zero(a[0]) || !plus_zero(a[1])) {
            if (bad < 10)
                printf("%s: %s taps %a %a %a %a %a %a %a %a at (%a, %a, %a): alpha %a / %a\n", what, f16 ? "f16" : "u8", t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7],
                       fx, fy, fz, a[0], a[1]);
            bad++;
            return;
        }
    }
}

static const uint16_t kF16Edges[] = {0x0000, 0x8000, 0x0001, 0x03FF, 0x8001, 0x0400, 0xBC00, 0xB8CD, 0xFBFF, 0x2519, 0x2E66, 0x2E67,
                                     0x2E65, 0x3B33, 0x3B34, 0x3C00, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0x7C01, 0xFC01, 0xFE00};
static const int kU8Edges[] = {0, 1, 24, 25, 26, 27, 128, 229, 230, 254, 255};

int main(int argc, char **argv) {
    if (argc == 2 && strcmp(argv[1], "taps") == 0) {
        for (uint32_t h = 0; h < 65536; h++) putchar(vk::builtin_tap_empty(h2f((uint16_t)h), true) ? '1' : '0');
        putchar('\n');
        for (int v = 0; v < 256; v++) putchar(vk::builtin_tap_empty((float)v, false) ? '1' : '0');
        putchar('\n');
        return 0;
    }
    const long cases = argc > 1 ? atol(argv[1]) : 100000;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    float t[8];
    // every f16 pattern as a uniform cell, and next to a 0 tap (in a drawn corner); every u8 value the same
    for (uint32_t h = 0; h < 65536; h++) {
        const float v = h2f((uint16_t)h);
        for (int b = 0; b < 8; b++) t[b] = v;
        check(t, true, "uniform");
        for (int b = 0; b < 8; b++) t[b] = 0.0f;
        t[rnd() % 8] = v;
        check(t, true, "next to 0");
    }
    for (int v = 0; v < 256; v++) {
        for (int b = 0; b < 8; b++) t[b] = (float)v;
        check(t, false, "uniform");
        for (int b = 0; b < 8; b++) t[b] = 0.0f;
        t[rnd() % 8] = (float)v;
        check(t, false, "next to 0");
    }
    // random cells of edge values (and, one tap in four, any pattern or value)
    const int nf = (int)(sizeof(kF16Edges) / sizeof(kF16Edges[0])), nu = (int)(sizeof(kU8Edges) / sizeof(kU8Edges[0]));
    for (long c = 0; c < cases; c++) {
        const bool f16 = c & 1;
        const int width = 1 + (int)(rnd() % (f16 ? nf : nu));  // draw from the first `width` edges: low, mostly empty, sets are common
        for (int b = 0; b < 8; b++) {
            if (f16) t[b] = h2f(rnd() % 4 == 0 ? (uint16_t)rnd() : kF16Edges[rnd() % width]);
            else t[b] = (float)(rnd() % 4 == 0 ? (int)(rnd() % 256) : kU8Edges[rnd() % width]);
        }
        check(t, f16, "edges");
    }
    printf("bad %ld of %ld (%ld empty)\n", bad, cells, empty);
    return bad ? 1 : 0;
}
