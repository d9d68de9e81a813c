// TEST INFRASTRUCTURE: host build of the geometry pass's shared header (vokselis_amd/csrc/vk_geom.hpp) under ASan + UBSan, against brute force.
// 1. vk::geom_flags_check, the flag-validation table of vk_render_geometry: every subset of NO_SKIP | SAFE | FORCE_SKIP | PROBE_ALWAYS is
//    accepted; VK_RENDER_FAST_WALK with nothing but accepted flags is refused as unsupported, with "isosurface" in the message; a word
//    with any other bit is refused as invalid.  Every single bit is walked first, then random words.
// 2. vk::geom_distance against long double: within 4 * 2^-24 of the sum of the three products' magnitudes (three roundings of terms no larger
//    than that sum, and the differences' own), and exactly the written operation order where that can be redone in double.
// 3. The miss record's bit pattern: (0, 0, 0, +inf), (0, 0, 0, 0); its t is not finite.
// 4. The record / pitch arithmetic of the read-back (geom_row_bytes, geom_surface_bytes, geom_pitch_ok, geom_dst_bytes, geom_record_offset)
//    against brute force: a surface of counted records is copied row by row into a destination of exactly geom_dst_bytes (ASan holds the
//    last row's end), with pitches from the row's own to larger ones and surfaces from 1 x 1; every record is then found at its offset.
// usage: geom_fuzz <cases> <seed>; prints "OK (<cases> cases)" or the first violations, and exits non-zero on any.
#include "vk_geom.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

static uint64_t state;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static float unit() { return (float)((rnd() >> 40) / 16777216.0); }  // [0, 1)
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static long bad = 0;
static void fail(long c, const char *what, double a, double b) { if (bad < 10) printf("case %ld: %s (%a, %a)\n", c, what, a, b); bad++; }

static void check_flags(long c, uint32_t flags) {
    const uint32_t ok_bits = VK_RENDER_NO_SKIP | VK_RENDER_SAFE | VK_RENDER_FORCE_SKIP | VK_RENDER_PROBE_ALWAYS;
    bool unsupported = true;
    const char *why = vk::geom_flags_check(flags, &unsupported);
    const bool other = (flags & ~(ok_bits | (uint32_t)VK_RENDER_FAST_WALK)) != 0, fast = (flags & VK_RENDER_FAST_WALK) != 0;
    if (!other && !fast) {
        if (why || unsupported) fail(c, "an accepted flag word is refused", flags, 0);
    } else if (other) {
        if (!why || unsupported) fail(c, "a word with another flag is not VK_ERR_INVALID", flags, 0);
    } else {
        if (!why || !unsupported || !strstr(why, "isosurface")) fail(c, "VK_RENDER_FAST_WALK is not VK_ERR_UNSUPPORTED with 'isosurface' in the message", flags, 0);
    }
}

static void check_distance(long c, const float q[3], const float eye[3], const float dir[3]) {
    const float got = vk::geom_distance(q[0], q[1], q[2], eye, dir);
    // the written order, redone: the differences are single f32 subtractions; the product of two floats is exact in double
    const float dx = q[0] - eye[0], dy = q[1] - eye[1], dz = q[2] - eye[2];
    const float m = (float)((double)dx * (double)dir[0]);
    const float want = fmaf(dz, dir[2], fmaf(dy, dir[1], m));
    if (bits(got) != bits(want)) fail(c, "t is not fma(dz, d.z, fma(dy, d.y, dx * d.x))", got, want);
    const long double exact = (long double)dx * dir[0] + (long double)dy * dir[1] + (long double)dz * dir[2];
    const long double mag = fabsl((long double)dx * dir[0]) + fabsl((long double)dy * dir[1]) + fabsl((long double)dz * dir[2]);
    if (fabsl((long double)got - exact) > 4.0L * 0x1p-24L * mag + 0x1p-140L) fail(c, "t is further from the exact dot product than three roundings allow", got, (double)exact);
}

static void check_surface(long c, uint32_t w, uint32_t h, size_t extra) {
    const size_t row = vk::geom_row_bytes(w), pitch = row + extra;
    if (row != (size_t)w * 32u || vk::geom_surface_bytes(w, h) != (size_t)w * h * 32u) fail(c, "row / surface bytes", (double)w, (double)h);
    if (!vk::geom_pitch_ok(w, pitch) || (row > 0 && vk::geom_pitch_ok(w, row - 1)) || (row >= 32 && vk::geom_pitch_ok(w, row - 32))) fail(c, "geom_pitch_ok", (double)w, (double)pitch);
    // brute force: the bytes a row-by-row copy touches, counted
    size_t touched_end = 0;
    for (uint32_t y = 0; y < h; y++) touched_end = (size_t)y * pitch + row;
    if (vk::geom_dst_bytes(w, h, pitch) != touched_end) fail(c, "geom_dst_bytes is not the end of the last row", (double)vk::geom_dst_bytes(w, h, pitch), (double)touched_end);
    std::vector<uint32_t> src((size_t)w * h * 8u);
    for (size_t i = 0; i < src.size(); i++) src[i] = (uint32_t)(i * 2654435761u + 12345u);
    std::vector<unsigned char> dst(vk::geom_dst_bytes(w, h, pitch), 0xAB);  // exactly as large: a copy past the last row's end is ASan's to find
    for (uint32_t y = 0; y < h; y++) memcpy(dst.data() + (size_t)y * pitch, reinterpret_cast<const unsigned char *>(src.data()) + (size_t)y * row, row);
    size_t counted = 0;  // records in row-major order
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++, counted++) {
            if (vk::geom_record_offset(x, y, row) != counted * 32u) fail(c, "a record's offset in the surface is not 32 * its row-major index", x, y);
            if (memcmp(dst.data() + vk::geom_record_offset(x, y, pitch), src.data() + counted * 8u, 32) != 0) fail(c, "a record is not at its offset in the read-back", x, y);
        }
    for (uint32_t y = 0; y + 1 < h; y++)  // the gap between rows is left alone
        for (size_t k = row; k < pitch; k++)
            if (dst[(size_t)y * pitch + k] != 0xAB) { fail(c, "the copy wrote between rows", y, (double)k); break; }
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 400;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!state) state = 1;
    static_assert(sizeof(vk_hit) == 36, "vk_hit is 36 bytes");
    static_assert(sizeof(vk::GeomDesc) == 16 && vk::kGeomRecordBytes == 32, "GeomDesc, the record");
    // 3. the miss record
    const float miss[8] = {0.0f, 0.0f, 0.0f, INFINITY, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < 8; i++)
        if (bits(miss[i]) != vk::kGeomMissBits[i]) fail(-3, "the miss record's bit pattern", i, vk::kGeomMissBits[i]);
    if (isfinite(miss[3]) || vk::kGeomMissBits[3] != 0x7f800000u) fail(-3, "the miss record's t is finite", miss[3], 0);
    // 1. the flag table: no flag, every single bit, every pair with an accepted flag, all accepted flags together
    check_flags(-1, 0);
    for (int b = 0; b < 32; b++) {
        check_flags(-1, 1u << b);
        check_flags(-1, (1u << b) | VK_RENDER_NO_SKIP);
        check_flags(-1, (1u << b) | vk::kGeomFlags);
        check_flags(-1, (1u << b) | VK_RENDER_FAST_WALK);
    }
    for (uint32_t s = 0; s < 16; s++) {  // every subset of the four accepted flags, alone and with FAST_WALK
        const uint32_t f = ((s & 1) ? VK_RENDER_NO_SKIP : 0) | ((s & 2) ? VK_RENDER_SAFE : 0) | ((s & 4) ? VK_RENDER_FORCE_SKIP : 0) | ((s & 8) ? VK_RENDER_PROBE_ALWAYS : 0);
        check_flags(-1, f);
        check_flags(-1, f | VK_RENDER_FAST_WALK);
    }
    // 4. the smallest surfaces, pitches at and above the row
    for (uint32_t w = 1; w <= 3; w++)
        for (uint32_t h = 1; h <= 3; h++)
            for (size_t extra : {(size_t)0, (size_t)1, (size_t)32, (size_t)100}) check_surface(-4, w, h, extra);
    if (vk::geom_dst_bytes(5, 0, 1000) != 0) fail(-4, "an empty surface reads back bytes", 0, 0);
    for (long c = 0; c < cases; c++) {
        for (int j = 0; j < 64; j++) {
            check_flags(c, (uint32_t)rnd());
            check_flags(c, (uint32_t)rnd() & (vk::kGeomFlags | VK_RENDER_FAST_WALK));
            // 2. q in and around the unit cube, the eye up to a few units away, a unit direction (and now and then an axis-aligned one)
            float q[3], eye[3], dir[3];
            double len = 0.0;
            for (int k = 0; k < 3; k++) {
                q[k] = unit() * 1.2f - 0.1f;
                eye[k] = (unit() - 0.5f) * 8.0f;
                dir[k] = (rnd() & 7) ? unit() - 0.5f : 0.0f;
                len += (double)dir[k] * dir[k];
            }
            if (len == 0.0) { dir[0] = 1.0f; len = 1.0; }
            for (int k = 0; k < 3; k++) dir[k] = (float)(dir[k] / sqrt(len));
            check_distance(c, q, eye, dir);
        }
        check_surface(c, 1 + (uint32_t)(rnd() % 40), 1 + (uint32_t)(rnd() % 24), (rnd() & 1) ? 0 : (size_t)(rnd() % 200));
    }
    if (bad) {
        printf("bad %ld\n", bad);
        return 1;
    }
    printf("OK (%ld cases)\n", cases);
    return 0;
}
