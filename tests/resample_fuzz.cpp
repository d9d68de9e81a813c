// resample_fuzz.cpp -- vk_resample.hpp on the host, under ASan + UBSan (a stand-alone program; tests/test_resample_fuzz_cpu.py builds and
// runs it): the integer geometry of the three rules over random extents up to 65535 and every ratio, the per-axis tables against the
// per-voxel functions and inside their array, the 64-bit offsets of a gather inside the source box and the output, the grid, and the
// request's validation.
//   resample_fuzz <cases> <seed>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vk_resample.hpp"

using namespace vk;

static uint64_t g_state;
static uint64_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            std::exit(1);                                  \
        }                                                  \
    } while (0)

// an extent: small ones, the edges of the range, anything
static uint32_t extent() {
    switch (below(6)) {
        case 0: return 1u + below(8);
        case 1: return 65535u - below(4);
        case 2: return 1u + below(300);
        case 3: return 1u << below(16);
        default: return 1u + below(65535);
    }
}

static int64_t floordiv(int64_t a, int64_t b) {
    int64_t q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) q--;
    return q;
}

// one axis: every j, or a sample of them on a long axis
static void check_axis(uint32_t nb, uint32_t n) {
    const uint32_t step = n > 4096u ? 1u + below(n / 2048u) : 1u;
    // NEAREST and LINEAR
    for (uint32_t j = 0; j < n; j += step) {
        const uint32_t i = resample_nearest(j, nb, n);
        CHECK(i < nb, "nearest %u of nb %u n %u: %u", j, nb, n, i);
        CHECK((int64_t)i == floordiv((2 * (int64_t)j + 1) * nb, 2 * (int64_t)n), "nearest %u nb %u n %u", j, nb, n);
        // the centre of output voxel j, (j + 0.5) nb / n, lies in [i, i + 1)
        CHECK((uint64_t)i * 2u * n <= (2u * (uint64_t)j + 1u) * nb && (2u * (uint64_t)j + 1u) * nb < ((uint64_t)i + 1u) * 2u * n, "nearest holds the centre");
        const ResampleLinearTap L = resample_linear(j, nb, n);
        CHECK(L.i0 < nb && L.i1 < nb && L.i0 <= L.i1 && L.i1 - L.i0 <= 1u, "linear taps %u %u of nb %u", L.i0, L.i1, nb);
        CHECK(L.f >= 0.0f && L.f < 1.0f, "linear f %g (j %u nb %u n %u)", (double)L.f, j, nb, n);
        const int64_t num = (2 * (int64_t)j + 1) * nb - n, den = 2 * (int64_t)n, fl = floordiv(num, den);
        CHECK((int64_t)L.i0 == (fl < 0 ? 0 : (fl > (int64_t)nb - 1 ? (int64_t)nb - 1 : fl)), "linear i0");
        CHECK(L.f == (float)((double)(num - fl * den) / (double)den), "linear f");
        if (nb == n) CHECK(L.i0 == j && L.f == 0.0f && i == j, "the identity");
    }
    // AREA: within the ratio cap
    if (!resample_area_ratio_ok(nb, n)) return;
    uint32_t expect_first = 0u;
    const bool all = step == 1u;
    for (uint32_t j = 0; j < n; j += all ? 1u : step) {
        const uint32_t k0 = resample_area_first(j, nb, n), k1 = resample_area_last(j, nb, n);
        CHECK(k0 <= k1 && k1 < nb, "area taps %u .. %u of nb %u", k0, k1, nb);
        CHECK(k1 - k0 + 1u <= kResampleMaxTaps, "area tap count %u (nb %u n %u)", k1 - k0 + 1u, nb, n);
        uint64_t sum = 0;
        for (uint32_t k = k0; k <= k1; k++) {
            const uint64_t o = resample_area_overlap(j, k, nb, n);
            CHECK(o > 0u, "area overlap 0 at j %u k %u nb %u n %u", j, k, nb, n);
            const float w = resample_area_weight(j, k, nb, n);
            CHECK(w > 0.0f && w <= 1.0f, "area weight %g", (double)w);
            sum += o;
        }
        CHECK(sum == nb, "area overlaps of j %u sum to %" PRIu64 ", not nb %u (n %u)", j, sum, nb, n);
        if (k0 > 0u) CHECK(resample_area_overlap(j, k0 - 1u, nb, n) == 0u, "a tap before the first");
        if (k1 + 1u < nb) CHECK(resample_area_overlap(j, k1 + 1u, nb, n) == 0u, "a tap behind the last");
        if (all) {  // consecutive ranges tile [0, nb) without a gap: the next starts at this one's last tap or right behind it
            CHECK(j == 0u ? k0 == 0u : (k0 == expect_first || k0 + 1u == expect_first), "area ranges: j %u starts at %u, the one before ended before %u", j, k0, expect_first);
            expect_first = k1 + 1u;
            if (j + 1u == n) CHECK(k1 == nb - 1u, "area ranges end at nb - 1");
        }
    }
}

// the tables of a call against the per-voxel functions; the words stay inside the array (ASan holds the vector's bounds)
static void check_tables(int mode, const uint32_t nb[3], const uint32_t n[3]) {
    ResampleAxis ax[3];
    const uint32_t words = resample_table_layout(mode, nb, n, ax);
    uint64_t expect = 0;
    for (int a = 0; a < 3; a++) {
        CHECK(ax[a].base == expect, "axis %d base", a);
        if (mode == VK_RESAMPLE_AREA) CHECK(ax[a].taps >= 1u && ax[a].taps <= kResampleMaxTaps, "axis %d taps %u", a, ax[a].taps);
        expect += resample_axis_words(mode, n[a], ax[a].taps);
    }
    CHECK(expect == words && expect < (1ull << 32), "table words");
    std::vector<uint32_t> t(words, 0xdeadbeefu);
    for (int a = 0; a < 3; a++) resample_table_fill(mode, ax[a], t.data());
    for (int a = 0; a < 3; a++) {
        const uint32_t *p = t.data() + ax[a].base;
        for (uint32_t j = 0; j < n[a]; j++) {
            if (mode == VK_RESAMPLE_NEAREST) CHECK(p[j] == resample_nearest(j, nb[a], n[a]), "nearest table");
            else if (mode == VK_RESAMPLE_LINEAR) {
                const ResampleLinearTap L = resample_linear(j, nb[a], n[a]);
                CHECK(p[3u * j] == L.i0 && p[3u * j + 1u] == L.i1 && p[3u * j + 2u] == filter_f32_bits(L.f), "linear table");
            } else {
                const uint32_t k0 = p[2u * j], c = p[2u * j + 1u];
                CHECK(k0 == resample_area_first(j, nb[a], n[a]) && c >= 1u && c <= ax[a].taps && k0 + c - 1u == resample_area_last(j, nb[a], n[a]), "area table");
                CHECK(k0 + c <= nb[a], "area taps inside the box");
                const uint32_t *w = p + 2u * (size_t)n[a] + (size_t)j * ax[a].taps;
                for (uint32_t k = 0; k < ax[a].taps; k++) CHECK(w[k] == (k < c ? filter_f32_bits(resample_area_weight(j, k0 + k, nb[a], n[a])) : 0u), "area weights");
            }
        }
    }
    for (uint32_t w : t) CHECK(mode == VK_RESAMPLE_AREA || w != 0xdeadbeefu, "a table word was not written");
}

// a box in a volume: the offsets of the gather's corners inside the source, of the output inside its array; the grid
static void check_offsets_and_grid() {
    uint32_t vol[3], lo[3], nb[3], n[3];
    for (int a = 0; a < 3; a++) {
        vol[a] = 1u + below(8192);
        lo[a] = below(vol[a]);
        nb[a] = 1u + below(vol[a] - lo[a]);
        n[a] = extent();
    }
    const uint64_t src = (uint64_t)vol[0] * vol[1] * vol[2], dst = (uint64_t)n[0] * n[1] * n[2];
    for (int corner = 0; corner < 8; corner++) {
        uint32_t j[3], s[3];
        for (int a = 0; a < 3; a++) {
            j[a] = (corner >> a) & 1 ? n[a] - 1u : 0u;
            s[a] = lo[a] + resample_linear(j[a], nb[a], n[a]).i1;
            CHECK(s[a] < lo[a] + nb[a] && s[a] < vol[a], "a source index leaves the box");
            CHECK(lo[a] + resample_nearest(j[a], nb[a], n[a]) < lo[a] + nb[a], "nearest leaves the box");
            if (resample_area_ratio_ok(nb[a], n[a])) CHECK(lo[a] + resample_area_last(j[a], nb[a], n[a]) < lo[a] + nb[a], "area leaves the box");
        }
        CHECK(voxel_index(s[0], s[1], s[2], vol[0], vol[1]) < src, "source offset");
        CHECK(voxel_index(j[0], j[1], j[2], n[0], n[1]) < dst, "output offset");
    }
    CHECK(voxel_index(n[0] - 1u, n[1] - 1u, n[2] - 1u, n[0], n[1]) == dst - 1u, "the last output offset");
    const uint32_t cap = below(3) ? 0u : 1u + below(5);
    const uint32_t tz = below(2) ? 1u : 4u;
    const ResampleGrid G = resample_grid(n[0], n[1], n[2], cap, tz);
    CHECK(G.blocks >= 1u && G.blocks <= kResampleMaxBlocks && (uint64_t)G.blocks * kResampleThreads < (1ull << 31), "grid %u", G.blocks);
    CHECK(!cap || (G.flat && G.blocks <= cap), "the cap");
    CHECK((uint64_t)G.ntx * kResampleTileX >= n[0] && (uint64_t)(G.ntx - 1u) * kResampleTileX < n[0], "tiles along x");
    CHECK((uint64_t)G.nty * kResampleTileY >= n[1] && (uint64_t)(G.nty - 1u) * kResampleTileY < n[1], "tiles along y");
    CHECK((uint64_t)G.ntz * tz >= n[2] && (uint64_t)(G.ntz - 1u) * tz < n[2], "tiles along z");
    CHECK(G.tiles == (uint64_t)G.ntx * G.nty * G.ntz, "tiles");
    if (G.flat) CHECK(G.trips * G.blocks >= G.tiles && (G.trips - 1u) * G.blocks < G.tiles, "trips %" PRIu64 " blocks %u tiles %" PRIu64, G.trips, G.blocks, G.tiles);
    else CHECK(G.trips == 1u && G.tiles * kResampleThreads <= (1ull << 31) && G.nty <= 65535u && G.ntz <= 65535u && G.ntx <= 1024u, "the three-dimensional grid: %u x %u x %u", G.ntx, G.nty, G.ntz);
    // the last tile a block reaches decomposes into indices inside the tile grid
    const uint64_t tile = G.tiles - 1u, rest = tile / G.ntx, z = rest / G.nty;
    CHECK(z < G.ntz && z * tz < n[2] && rest - z * G.nty < G.nty && tile - rest * G.ntx < G.ntx, "the last tile");
}

static void check_validation() {
    vk_resample_request r{};
    r.mode = (int32_t)below(3);
    r.flags = VK_RESAMPLE_INSTALL;
    r.format = VK_RESAMPLE_KEEP_FORMAT;
    r.layout = VK_LAYOUT_AUTO;
    CHECK(resample_validate(nullptr, true) != nullptr, "NULL");
    CHECK(resample_validate(&r, false) == nullptr && resample_validate(&r, true) == nullptr, "a plain request");
    vk_resample_request b = r;
    b.mode = 3 + (int32_t)below(100);
    CHECK(resample_validate(&b, true), "mode");
    b = r; b.mode = -1;
    CHECK(resample_validate(&b, true), "mode -1");
    b = r; b.flags |= 8u << below(28);
    CHECK(resample_validate(&b, true), "flag");
    b = r; b.format = VK_FMT_RGBA16F_PAIR;
    CHECK(resample_validate(&b, true), "RGBA16F_PAIR");
    b = r; b.format = 4 + (int32_t)below(100);
    CHECK(resample_validate(&b, true), "format");
    b = r; b.format = -2;
    CHECK(resample_validate(&b, true), "format -2");
    b = r; b.dims[below(3)] = 65536u + below(1000);
    CHECK(resample_validate(&b, true), "extent");
    b = r; b.dims[below(3)] = 65535u;
    CHECK(!resample_validate(&b, true), "extent 65535");
    b = r; b.flags = 0u;
    CHECK(resample_validate(&b, false) && !resample_validate(&b, true), "nowhere");
    b = r; b.layout = 7 + (int32_t)below(10);
    CHECK(resample_validate(&b, true), "layout");
    b.flags = 0u;
    CHECK(!resample_validate(&b, true), "layout is read with INSTALL only");
    b = r; b.flags |= VK_RESAMPLE_WINDOW; b.lo = 0.25f; b.hi = 0.5f;
    CHECK(!resample_validate(&b, true), "window");
    b.hi = 0.25f;
    CHECK(resample_validate(&b, true), "lo == hi");
    b.hi = INFINITY;
    CHECK(resample_validate(&b, true), "hi inf");
    b.hi = 0.5f; b.lo = NAN;
    CHECK(resample_validate(&b, true), "lo NaN");
    b.flags &= ~(uint32_t)VK_RESAMPLE_WINDOW;
    CHECK(!resample_validate(&b, true), "lo, hi are read with WINDOW only");
    // the plan
    ResamplePlan P;
    int status = 0;
    vk_voxel_box B{1u, 2u, 3u, 1u + 32u, 2u + 33u, 3u + 5u};
    b = r; b.mode = VK_RESAMPLE_AREA; b.dims[0] = 2u; b.dims[1] = 3u;
    CHECK(!resample_plan(&b, B, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED_PAIRS, P, status), "ratio 16 and 11");
    CHECK(P.nb[0] == 32u && P.nb[1] == 33u && P.nb[2] == 5u && P.n[0] == 2u && P.n[1] == 3u && P.n[2] == 5u && !P.map && P.layout == VK_LAYOUT_PACKED_PAIRS && P.format == VK_FMT_R8_UNORM, "plan");
    b.dims[1] = 2u;
    CHECK(resample_plan(&b, B, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED, P, status) && status == VK_ERR_UNSUPPORTED, "ratio 16 plus a voxel");
    b.mode = VK_RESAMPLE_LINEAR;
    CHECK(!resample_plan(&b, B, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED, P, status), "LINEAR has no cap");
    b.format = VK_FMT_R16_UNORM;
    CHECK(!resample_plan(&b, B, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED_PAIRS, P, status) && P.layout == VK_LAYOUT_PACKED && P.map && P.a == 257.0f && P.b == 0.0f, "AUTO leaves PACKED_PAIRS for u16");
    b.layout = VK_LAYOUT_PACKED_PAIRS;
    CHECK(resample_plan(&b, B, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED, P, status) && status == VK_ERR_UNSUPPORTED, "PACKED_PAIRS by name for u16");
    b.layout = VK_LAYOUT_STAGED;
    CHECK(resample_plan(&b, B, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED, P, status) && status == VK_ERR_UNSUPPORTED, "STAGED for u16");
    b.format = VK_FMT_R8_UNORM; b.layout = VK_LAYOUT_AUTO; b.dims[2] = 8193u;
    CHECK(resample_plan(&b, B, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED, P, status) && status == VK_ERR_UNSUPPORTED, "an install above 8192");
    b.flags = 0u;
    CHECK(!resample_plan(&b, B, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED, P, status) && P.layout == 0, "dense_out alone above 8192");
    vk_voxel_box E{4u, 4u, 4u, 4u, 9u, 9u};
    CHECK(resample_plan(&r, E, VK_FMT_R8_UNORM, VK_LAYOUT_PACKED, P, status) && status == VK_ERR_INVALID, "an empty box");
    b = r; b.flags |= VK_RESAMPLE_WINDOW; b.lo = 0.0f; b.hi = 1e-45f; b.format = VK_FMT_R16_UNORM;
    CHECK(resample_plan(&b, B, VK_FMT_R16_FLOAT, VK_LAYOUT_PACKED, P, status) && status == VK_ERR_INVALID, "a that overflows f32");
    b.lo = 0.25f; b.hi = 0.75f; b.format = VK_FMT_R8_UNORM;
    CHECK(!resample_plan(&b, B, VK_FMT_R16_UNORM, VK_LAYOUT_LINEAR, P, status) && P.map && P.a == (float)(255.0 / (0.5 * 65535.0)) && P.b == -127.5f, "the map's constants");
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 200;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!g_state) g_state = 1;
    // every ratio of small extents, exhaustively
    for (uint32_t nb = 1; nb <= 40u; nb++)
        for (uint32_t n = 1; n <= 40u; n++) check_axis(nb, n);
    // the ratio cap's edge
    for (uint32_t n = 1; n <= 64u; n++) {
        CHECK(resample_area_ratio_ok(16u * n, n) && !resample_area_ratio_ok(16u * n + 1u, n), "the cap at n %u", n);
        check_axis(16u * n, n);
        CHECK(resample_area_max_taps(16u * n, n) == 16u, "16 taps at ratio 16");
        if (n > 1u) CHECK(resample_area_max_taps(16u * n - 1u, n) <= kResampleMaxTaps, "17 taps at most");
    }
    for (int c = 0; c < cases; c++) {
        uint32_t nb = extent(), n = extent();
        if (below(4) == 0u) n = nb;                                  // the identity
        if (below(4) == 0u) {                                        // an integer ratio, up to the cap
            const uint32_t ratio = 1u + below(16);
            if ((uint64_t)n * ratio <= 65535u) nb = n * ratio;
        }
        check_axis(nb, n);
        uint32_t nbs[3], ns[3];
        for (int a = 0; a < 3; a++) { nbs[a] = 1u + below(200); ns[a] = 1u + below(200); }
        if (below(3) == 0u) { nbs[below(3)] = extent(); ns[below(3)] = extent(); }
        int mode = (int)below(3);
        for (int a = 0; a < 3; a++)
            if (mode == VK_RESAMPLE_AREA && !resample_area_ratio_ok(nbs[a], ns[a])) mode = VK_RESAMPLE_LINEAR;
        check_tables(mode, nbs, ns);
        check_offsets_and_grid();
        check_validation();
    }
    // the unrolled footprint's condition: exactly r taps on every axis for every j
    for (uint32_t r = 1; r <= 5u; r++)
        for (uint32_t n = 1; n <= 9u; n++) {
            const uint32_t nbs[3] = {r * n, r * (n + 1u), r * 7u}, ns[3] = {n, n + 1u, 7u}, off[3] = {r * n + 1u, r * (n + 1u), r * 7u};
            CHECK(resample_uniform_taps(nbs, ns) == (r >= 2u && r <= 4u ? r : 0u), "uniform taps at ratio %u", r);
            CHECK(resample_uniform_taps(off, ns) == 0u || off[0] / ns[0] != r, "a ratio that is no integer");
            if (resample_uniform_taps(nbs, ns))
                for (int a = 0; a < 3; a++)
                    for (uint32_t j = 0; j < ns[a]; j++)
                        CHECK(resample_area_first(j, nbs[a], ns[a]) == j * r && resample_area_last(j, nbs[a], ns[a]) == j * r + r - 1u, "r taps from j r");
        }
    // the store rule's NaN
    CHECK(resample_store_unorm(NAN, 255.0f) == 0u && resample_store_unorm(INFINITY, 255.0f) == 255u && resample_store_unorm(-INFINITY, 65535.0f) == 0u && resample_store_unorm(2.5f, 255.0f) == 2u &&
              resample_store_unorm(3.5f, 255.0f) == 4u, "the store rule");
    CHECK(resample_lerp(3.0f, INFINITY, 0.0f) == 3.0f, "an exact hit does not meet its neighbour");
    std::printf("OK (%d cases)\n", cases);
    return 0;
}
