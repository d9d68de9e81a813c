// TEST INFRASTRUCTURE: host build of the slice pass's shared header (vokselis_amd/csrc/vk_slice.hpp) under ASan + UBSan, against brute force.
// 1. vk::slice_validate, the validation table of vk_render_slice: a NULL slice, a component of origin / du / dv that is not finite or beyond
//    +-VK_SLICE_MAX_COORD (the bound itself is accepted), samples outside 1 .. 256, dn's components and reduce checked under samples > 1 and
//    ignored under samples == 1; an accepted slice arrives in the descriptor as given (dn zeroed, reduce MAX under samples == 1).
// 2. rn = (float)(1.0 / (double)samples) for every samples, and the window: k1, k2, umax, imax of tf_constants for a table and for the grey ramp.
// 3. vk::slab_offset for every samples up to 256 and every k below it: exactly k - (samples - 1) / 2 (compared in double), the offsets of a
//    slab symmetric about 0 and one apart.
// 4. vk::slice_position against long double: within 3 * 2^-24 of |origin| + |px du| + |py dv| (the conversions are exact; two fused
//    operations round once each, to values no larger than that sum up to a rounding -- held to three roundings), and exactly the written
//    operation order; vk::slice_inside on the faces, one ulp outside them and on NaN; the reductions' steps on NaN and signed zeros.
// 5. The record / pitch arithmetic of the read-back (slice_row_bytes, slice_surface_bytes, slice_pitch_ok, slice_dst_bytes,
//    slice_record_offset) against brute force, as tests/geom_fuzz.cpp does for the geometry surface; slice_tile_clip against a pixel count.
// usage: slice_fuzz <cases> <seed>; prints "OK (<cases> cases)" or the first violations, and exits non-zero on any.
#include "vk_slice.hpp"

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

static vk_slice good_slice() {
    vk_slice s;
    memset(&s, 0, sizeof s);
    for (int i = 0; i < 3; i++) { s.origin[i] = 0.25f * (float)i; s.du[i] = 0.01f; s.dv[i] = -0.02f; s.dn[i] = 0.003f; }
    s.samples = 1;
    s.reduce = VK_SLAB_MAX;
    return s;
}

static bool accepted(const vk_slice &s) {
    vk::SliceDesc D;
    memset(&D, 0, sizeof D);
    return vk::slice_validate(&s, 0, 0.0f, 1.0f, vk::SCALE_R8, D) == nullptr;
}

static void check_validation(long c) {
    vk::SliceDesc D;
    memset(&D, 0, sizeof D);
    if (!vk::slice_validate(nullptr, 0, 0.0f, 1.0f, vk::SCALE_R8, D)) fail(c, "a NULL slice is accepted", 0, 0);
    if (!accepted(good_slice())) fail(c, "a plain slice is refused", 0, 0);
    const float bad_values[] = {NAN, INFINITY, -INFINITY, 1.0000001e6f, -1.0000001e6f, 3.0e38f};
    const float ok_values[] = {VK_SLICE_MAX_COORD, -VK_SLICE_MAX_COORD, 0.0f, -0.0f, 1.0e-45f, 123456.0f};
    for (int vec = 0; vec < 4; vec++)
        for (int i = 0; i < 3; i++) {
            for (float v : bad_values)
                for (uint32_t samples : {1u, 2u}) {
                    vk_slice s = good_slice();
                    s.samples = samples;
                    (vec == 0 ? s.origin : vec == 1 ? s.du : vec == 2 ? s.dv : s.dn)[i] = v;
                    const bool want_refused = vec < 3 || samples > 1;  // dn is ignored under samples == 1
                    if (accepted(s) == want_refused) fail(c, "a bad component: wrong verdict", vec, samples);
                }
            for (float v : ok_values) {
                vk_slice s = good_slice();
                s.samples = 2;
                (vec == 0 ? s.origin : vec == 1 ? s.du : vec == 2 ? s.dv : s.dn)[i] = v;
                if (!accepted(s)) fail(c, "a component within the bounds is refused", vec, v);
            }
        }
    for (uint32_t samples : {0u, 257u, 258u, 1000u, 0x80000000u, 0xffffffffu}) {
        vk_slice s = good_slice();
        s.samples = samples;
        if (accepted(s)) fail(c, "samples outside 1 .. 256 are accepted", samples, 0);
    }
    for (int32_t reduce : {-1, 3, 4, 255, INT32_MIN, INT32_MAX}) {
        vk_slice s = good_slice();
        s.reduce = reduce;
        if (!accepted(s)) fail(c, "reduce is not ignored under samples == 1", reduce, 0);
        s.samples = 2;
        if (accepted(s)) fail(c, "an unknown reduce is accepted under samples > 1", reduce, 0);
    }
    for (uint32_t samples = 1; samples <= (uint32_t)VK_SLICE_MAX_SAMPLES; samples++)
        for (int32_t reduce : {VK_SLAB_MAX, VK_SLAB_MIN, VK_SLAB_MEAN}) {
            vk_slice s = good_slice();
            s.samples = samples;
            s.reduce = reduce;
            memset(&D, 0xAB, sizeof D);
            if (vk::slice_validate(&s, 0, 0.0f, 1.0f, vk::SCALE_U16, D)) { fail(c, "an accepted (samples, reduce) pair is refused", samples, reduce); continue; }
            // 2. rn and the descriptor
            if (bits(D.rn) != bits((float)(1.0 / (double)samples))) fail(c, "rn is not (float)(1.0 / (double)samples)", D.rn, samples);
            if (D.samples != samples || D.reduce != (samples > 1 ? reduce : (int32_t)VK_SLAB_MAX)) fail(c, "samples / reduce of the descriptor", samples, reduce);
            for (int i = 0; i < 3; i++) {
                if (bits(D.origin[i]) != bits(s.origin[i]) || bits(D.du[i]) != bits(s.du[i]) || bits(D.dv[i]) != bits(s.dv[i])) fail(c, "the plane of the descriptor", i, 0);
                if (bits(D.dn[i]) != bits(samples > 1 ? s.dn[i] : 0.0f)) fail(c, "dn of the descriptor", i, samples);
            }
            float k1, k2;
            vk::tf_constants(2, 0.0f, 1.0f, vk::SCALE_U16, k1, k2);
            if (bits(D.k1) != bits(k1) || bits(D.k2) != bits(k2) || D.umax != 1.0f || D.imax != 0) fail(c, "the grey ramp's window", D.k1, D.k2);
        }
    for (uint32_t n : {2u, 3u, 17u, 256u})
        for (vk::SampleScale sc : {vk::SCALE_VALUE, vk::SCALE_R8, vk::SCALE_U16}) {
            const vk_slice s = good_slice();
            float k1, k2;
            vk::tf_constants(n, -0.5f, 1.5f, sc, k1, k2);
            if (vk::slice_validate(&s, n, -0.5f, 1.5f, sc, D) || bits(D.k1) != bits(k1) || bits(D.k2) != bits(k2) || D.umax != (float)(n - 1u) || D.imax != (int32_t)n - 2)
                fail(c, "the table's window", n, (double)sc);
        }
}

static void check_slab_offsets(long c) {
    for (uint32_t samples = 1; samples <= (uint32_t)VK_SLICE_MAX_SAMPLES; samples++)
        for (uint32_t k = 0; k < samples; k++) {
            const float w = vk::slab_offset(k, samples);
            if ((double)w != (double)k - 0.5 * (double)(samples - 1u)) fail(c, "slab_offset is not exact", k, samples);
            if (bits(w + 0.0f) != bits(-vk::slab_offset(samples - 1u - k, samples) + 0.0f)) fail(c, "a slab's offsets are not symmetric about 0", k, samples);
            if (k + 1u < samples && vk::slab_offset(k + 1u, samples) - w != 1.0f) fail(c, "a slab's offsets are not one apart", k, samples);
        }
}

static void check_position(long c, float origin, float du, float dv, uint32_t px, uint32_t py) {
    const float got = vk::slice_position(origin, du, dv, px, py);
    const float want = fmaf((float)py, dv, fmaf((float)px, du, origin));
    if (bits(got) != bits(want)) fail(c, "P is not fma((float)py, dv, fma((float)px, du, origin))", got, want);
    const long double exact = (long double)origin + (long double)px * du + (long double)py * dv;
    const long double mag = fabsl((long double)origin) + fabsl((long double)px * du) + fabsl((long double)py * dv);
    if (fabsl((long double)got - exact) > 3.0L * 0x1p-24L * mag + 0x1p-149L) fail(c, "P is further from the exact position than three roundings allow", got, (double)exact);
}

static void check_inside_and_steps(long c) {
    const float lo[3] = {0.0f, 0.25f, 0.0f}, hi[3] = {1.0f, 0.75f, 1.0f};
    const float below0 = nextafterf(0.0f, -1.0f), above1 = nextafterf(1.0f, 2.0f);
    if (!vk::slice_inside(0.0f, 0.25f, 1.0f, lo, hi) || !vk::slice_inside(1.0f, 0.75f, 0.0f, lo, hi) || !vk::slice_inside(-0.0f, 0.5f, 0.5f, lo, hi)) fail(c, "a face is outside", 0, 0);
    if (vk::slice_inside(below0, 0.5f, 0.5f, lo, hi) || vk::slice_inside(0.5f, 0.5f, above1, lo, hi) || vk::slice_inside(0.5f, nextafterf(0.25f, 0.0f), 0.5f, lo, hi) ||
        vk::slice_inside(0.5f, nextafterf(0.75f, 1.0f), 0.5f, lo, hi))
        fail(c, "one ulp outside is inside", 0, 0);
    if (vk::slice_inside(NAN, 0.5f, 0.5f, lo, hi) || vk::slice_inside(0.5f, NAN, 0.5f, lo, hi) || vk::slice_inside(0.5f, 0.5f, NAN, lo, hi)) fail(c, "a NaN is inside", 0, 0);
    // the reductions: a NaN is passed over, the first of two equal zeros stays, all NaN leaves the start
    float M = -INFINITY, m = INFINITY;
    for (float x : {NAN, NAN}) { M = vk::slab_max_step(M, x); m = vk::slab_min_step(m, x); }
    if (M != -INFINITY || m != INFINITY) fail(c, "all-NaN slabs leave -inf / +inf", M, m);
    for (float x : {NAN, -0.0f, 0.0f, NAN, -3.0f, 2.0f}) { M = vk::slab_max_step(M, x); m = vk::slab_min_step(m, x); }
    if (M != 2.0f || m != -3.0f) fail(c, "max / min over NaNs", M, m);
    if (bits(vk::slab_max_step(vk::slab_max_step(-INFINITY, -0.0f), 0.0f)) != bits(-0.0f) || bits(vk::slab_min_step(vk::slab_min_step(INFINITY, 0.0f), -0.0f)) != bits(0.0f))
        fail(c, "of two zeros the first stays", 0, 0);
    if (bits(vk::slab_mean_step(0.0f, -0.0f)) != bits(0.0f) || vk::slab_mean_step(1.0f, 0x1p-30f) != 1.0f || !isnan(vk::slab_mean_step(1.0f, NAN))) fail(c, "the mean's step is acc + x", 0, 0);
}

static void check_surface(long c, uint32_t w, uint32_t h, size_t extra) {
    const size_t row = vk::slice_row_bytes(w), pitch = row + extra;
    if (row != (size_t)w * 8u || vk::slice_surface_bytes(w, h) != (size_t)w * h * 8u) fail(c, "row / surface bytes", (double)w, (double)h);
    if (!vk::slice_pitch_ok(w, pitch) || (row > 0 && vk::slice_pitch_ok(w, row - 1)) || (row >= 8 && vk::slice_pitch_ok(w, row - 8))) fail(c, "slice_pitch_ok", (double)w, (double)pitch);
    size_t touched_end = 0;  // brute force: the bytes a row-by-row copy touches
    for (uint32_t y = 0; y < h; y++) touched_end = (size_t)y * pitch + row;
    if (vk::slice_dst_bytes(w, h, pitch) != touched_end) fail(c, "slice_dst_bytes is not the end of the last row", (double)vk::slice_dst_bytes(w, h, pitch), (double)touched_end);
    std::vector<uint32_t> src((size_t)w * h * 2u);
    for (size_t i = 0; i < src.size(); i++) src[i] = (uint32_t)(i * 2654435761u + 12345u);
    std::vector<unsigned char> dst(vk::slice_dst_bytes(w, h, pitch), 0xAB);  // exactly as large: a copy past the last row's end is ASan's to find
    for (uint32_t y = 0; y < h; y++) memcpy(dst.data() + (size_t)y * pitch, reinterpret_cast<const unsigned char *>(src.data()) + (size_t)y * row, row);
    size_t counted = 0;  // records in row-major order
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++, counted++) {
            if (vk::slice_record_offset(x, y, row) != counted * 8u) fail(c, "a record's offset in the surface is not 8 * its row-major index", x, y);
            if (memcmp(dst.data() + vk::slice_record_offset(x, y, pitch), src.data() + counted * 2u, 8) != 0) fail(c, "a record is not at its offset in the read-back", x, y);
        }
    for (uint32_t y = 0; y + 1 < h; y++)  // the gap between rows is left alone
        for (size_t k = row; k < pitch; k++)
            if (dst[(size_t)y * pitch + k] != 0xAB) { fail(c, "the copy wrote between rows", y, (double)k); break; }
}

static void check_tile_clip(long c, int32_t tx, int32_t ty, uint32_t tw, uint32_t th, uint32_t W, uint32_t H) {
    uint32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    const bool any = vk::slice_tile_clip(tx, ty, tw, th, W, H, x0, y0, x1, y1);
    long count = 0;  // brute force over the backbuffer's pixels
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const bool in_tile = (int64_t)x >= tx && (int64_t)x < (int64_t)tx + tw && (int64_t)y >= ty && (int64_t)y < (int64_t)ty + th;
            count += in_tile;
            if (in_tile && !(any && x >= x0 && x < x1 && y >= y0 && y < y1)) fail(c, "a pixel of the tile is left out", x, y);
        }
    if (any != (count > 0) || (any && (long)(x1 - x0) * (long)(y1 - y0) != count) || (any && (x1 > W || y1 > H))) fail(c, "slice_tile_clip is not the tile on the backbuffer", tx, ty);
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 400;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!state) state = 1;
    static_assert(sizeof(vk_slice) == 56 && sizeof(vk_slice_sample) == 20, "vk_slice is 56 bytes, vk_slice_sample 20");
    static_assert(sizeof(vk::SliceDesc) % 16 == 0 && vk::kSliceRecordBytes == 8, "SliceDesc, the record");
    check_validation(-1);
    check_slab_offsets(-3);
    check_inside_and_steps(-4);
    for (uint32_t w = 1; w <= 3; w++)
        for (uint32_t h = 1; h <= 3; h++)
            for (size_t extra : {(size_t)0, (size_t)1, (size_t)8, (size_t)100}) check_surface(-5, w, h, extra);
    if (vk::slice_dst_bytes(5, 0, 1000) != 0) fail(-5, "an empty surface reads back bytes", 0, 0);
    check_tile_clip(-5, INT32_MIN, INT32_MIN, 0xffffffffu, 0xffffffffu, 5, 4);
    check_tile_clip(-5, INT32_MAX, INT32_MAX, 0xffffffffu, 0xffffffffu, 5, 4);
    check_tile_clip(-5, -3, -2, 3, 2, 5, 4);
    check_tile_clip(-5, 0, 0, 0, 7, 5, 4);
    for (long c = 0; c < cases; c++) {
        for (int j = 0; j < 64; j++) {
            // 4. planes in and around the unit cube, steps of a pixel of a small to a large frame, and now and then the bounds' magnitude
            const float scale = (rnd() & 15) ? 1.0f : VK_SLICE_MAX_COORD;
            const float origin = (unit() * 3.0f - 1.0f) * scale, du = (rnd() & 7) ? (unit() - 0.5f) * 0.05f * scale : 0.0f, dv = (rnd() & 7) ? (unit() - 0.5f) * 0.05f * scale : 0.0f;
            check_position(c, origin, du, dv, (uint32_t)(rnd() % 8192), (uint32_t)(rnd() % 8192));
        }
        check_surface(c, 1 + (uint32_t)(rnd() % 40), 1 + (uint32_t)(rnd() % 24), (rnd() & 1) ? 0 : (size_t)(rnd() % 200));
        check_tile_clip(c, (int32_t)(rnd() % 60) - 20, (int32_t)(rnd() % 50) - 20, (uint32_t)(rnd() % 50), (uint32_t)(rnd() % 40), 1 + (uint32_t)(rnd() % 40), 1 + (uint32_t)(rnd() % 24));
    }
    if (bad) {
        printf("bad %ld\n", bad);
        return 1;
    }
    printf("OK (%ld cases)\n", cases);
    return 0;
}
