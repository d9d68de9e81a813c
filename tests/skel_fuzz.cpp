// skel_fuzz.cpp -- vk_skel.hpp on the host, under ASan + UBSan: the library's own request validation in its order, the simple-point
// test against a plain flood fill over explicit neighbour lists, the mask's bit order against label_offset, the subfields, the tile and
// halo arithmetic, and the thin kernel's iterations replayed on the host.  A stand-alone program:
//     skel_fuzz CASES SEED [all]
// all: the simple-point test over all 2^26 masks (the unsanitized build); without it every mask of popcount <= 4 or >= 22 plus 2^22
// random ones.  Per case a random volume, set, box, mode and iteration cap: the sub-passes over an active-tile set as the device runs
// them -- tiles in a shuffled order, a tile's voxels in a shuffled order, stores going to the shared state at once, halo bytes taken at
// random from the state of before the sub-pass or of now (both are what a workgroup may load) -- against the sequential restatement
// (tests/skel_restatement.c, linked in).
#include "vk_skel.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace vk;

extern "C" int skel_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, float lo, float hi, int mode, uint32_t max_iterations, int fill_in_on, float fill_in,
                            float fill_out, const uint32_t *box, uint8_t *classes, void *dense, uint64_t *result);

static uint64_t g_state;
static uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }
template <class T>
static void shuffle(std::vector<T> &v) {
    for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd_below((uint32_t)i)]);
}

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static void check_validation() {
    vk_skeleton_request ok;
    std::memset(&ok, 0, sizeof ok);
    ok.lo = 0.3f; ok.hi = INFINITY;
    CHECK(skel_validate(&ok, true, false, false) == nullptr && skel_validate(&ok, false, true, false) == nullptr && skel_validate(&ok, false, false, true) == nullptr, "a plain request stands");
    CHECK(skel_validate(nullptr, true, true, true) != nullptr, "NULL");
    // the order: every request below carries every later fault as well, and the first is the one reported
    struct Step { const char *word; void (*change)(vk_skeleton_request &); };
    const Step steps[] = {
        {"NaN", [](vk_skeleton_request &r) { r.hi = NAN; }},
        {"lo > hi", [](vk_skeleton_request &r) { r.lo = 1.0f; r.hi = 0.5f; }},
        {"unknown mode", [](vk_skeleton_request &r) { r.mode = 2u; }},
        {"unknown flag", [](vk_skeleton_request &r) { r.flags = 8u | VK_SKEL_FILL_IN; }},
        {"pad must be 0", [](vk_skeleton_request &r) { r.pad = 1u; }},
        {"fill_out is not finite", [](vk_skeleton_request &r) { r.fill_out = INFINITY; }},
        {"fill_in is not finite", [](vk_skeleton_request &r) { r.fill_in = NAN; r.flags |= VK_SKEL_FILL_IN; }},
    };
    const size_t n_steps = sizeof steps / sizeof steps[0];
    for (size_t first = 0; first < n_steps; first++) {
        vk_skeleton_request r = ok;
        for (size_t k = n_steps; k-- > first;) steps[k].change(r);
        const char *why = skel_validate(&r, false, false, false);
        CHECK(why && std::strstr(why, steps[first].word), "fault %zu: got \"%s\", expected \"%s\"", first, why ? why : "(accepted)", steps[first].word);
    }
    const char *why = skel_validate(&ok, false, false, false);
    CHECK(why && std::strstr(why, "the result would go nowhere"), "nothing requested comes last");
    vk_skeleton_request r = ok;
    r.flags = VK_SKEL_INSTALL | VK_SKEL_CLIP_BOX;
    CHECK(skel_validate(&r, false, false, false) == nullptr, "INSTALL alone is a request");
    r = ok; r.fill_in = NAN;
    CHECK(skel_validate(&r, true, false, false) == nullptr, "fill_in counts under its flag only");
    r = ok; r.mode = VK_SKEL_KERNEL; r.max_iterations = 0xffffffffu; r.flags = VK_SKEL_FILL_IN; r.fill_in = -3.0f; r.lo = r.hi = -INFINITY;
    CHECK(skel_validate(&r, true, false, false) == nullptr, "kernel mode, any cap, any finite fill, lo == hi");
    for (uint32_t mode : {2u, 3u, 0x80000000u, 0xffffffffu}) { r = ok; r.mode = mode; CHECK(skel_validate(&r, true, false, false) != nullptr, "mode %u", mode); }
    for (uint32_t flags : {8u, 16u, 0x80000000u}) { r = ok; r.flags = flags; CHECK(skel_validate(&r, true, false, false) != nullptr, "flags %u", flags); }
}

// ---- the simple-point test, written out: lists of neighbours, a queue ------------------------------------------------------------------
static int g_d[26][3];
struct Neighbours { int n = 0, at[26]; void push_back(int b) { at[n++] = b; } };
static Neighbours g_adj26[26], g_adj6[26];
static void build_lists() {
    for (uint32_t k = 0; k < 26u; k++) label_offset(k < 13u ? k : k + 1u, g_d[k][0], g_d[k][1], g_d[k][2]);
    for (int a = 0; a < 26; a++)
        for (int b = 0; b < 26; b++) {
            const int ex = std::abs(g_d[a][0] - g_d[b][0]), ey = std::abs(g_d[a][1] - g_d[b][1]), ez = std::abs(g_d[a][2] - g_d[b][2]);
            if (a != b && std::max(ex, std::max(ey, ez)) == 1) g_adj26[a].push_back(b);
            const int la = std::abs(g_d[a][0]) + std::abs(g_d[a][1]) + std::abs(g_d[a][2]), lb = std::abs(g_d[b][0]) + std::abs(g_d[b][1]) + std::abs(g_d[b][2]);
            if (ex + ey + ez == 1 && la <= 2 && lb <= 2) g_adj6[a].push_back(b);
        }
}
static int plain_components(const bool *member, const Neighbours *adj, bool faces_only) {
    bool seen[26] = {};
    int n = 0;
    for (int s = 0; s < 26; s++) {
        if (!member[s] || seen[s]) continue;
        if (faces_only && std::abs(g_d[s][0]) + std::abs(g_d[s][1]) + std::abs(g_d[s][2]) != 1) continue;
        n++;
        int queue[26], head = 0, tail = 0;
        queue[tail++] = s; seen[s] = true;
        while (head < tail) {
            const int c = queue[head++];
            for (int e = 0; e < adj[c].n; e++) {
                const int u = adj[c].at[e];
                if (member[u] && !seen[u]) { seen[u] = true; queue[tail++] = u; }
            }
        }
    }
    return n;
}
static bool plain_simple(uint32_t m) {
    bool set[26], open[26];
    for (int k = 0; k < 26; k++) {
        set[k] = (m >> k) & 1u;
        open[k] = !set[k] && std::abs(g_d[k][0]) + std::abs(g_d[k][1]) + std::abs(g_d[k][2]) <= 2;
    }
    return plain_components(set, g_adj26, false) == 1 && plain_components(open, g_adj6, true) == 1;
}
static void check_simple(bool all) {
    uint64_t tested = 0, simple = 0;
    auto one = [&](uint32_t m) {
        const bool want = plain_simple(m), got = skel_simple(m);
        CHECK(want == got, "mask 0x%07x: the flood by shifts says %d, the plain flood fill %d", m, (int)got, (int)want);
        CHECK(skel_compress(skel_expand(m)) == m && (skel_expand(m) & (1u << kLabelCentre)) == 0u && skel_popcount(m) == (uint32_t)__builtin_popcount(m), "mask 0x%07x: the two forms", m);
        CHECK(skel_line_end(m) == (__builtin_popcount(m) == 1), "mask 0x%07x: line end", m);
        tested++; simple += got;
    };
    if (all) {
        for (uint32_t m = 0; m < (1u << 26); m++) one(m);
    } else {
        for (uint32_t a = 0; a < 26u; a++)
            for (uint32_t b = a; b < 26u; b++)
                for (uint32_t c = b; c < 26u; c++)
                    for (uint32_t d = c; d < 26u; d++) {  // every mask of at most 4 bits (repeats fold), and its complement
                        const uint32_t m = (1u << a) | (1u << b) | (1u << c) | (1u << d);
                        one(m); one(~m & ((1u << 26) - 1u));
                    }
        one(0u); one((1u << 26) - 1u);
        for (uint32_t k = 0; k < (1u << 22); k++) one((uint32_t)rnd() & ((1u << 26) - 1u));
    }
    CHECK(!skel_simple(0u) && !skel_simple((1u << 26) - 1u), "an isolated voxel and an interior voxel are not simple");
    for (uint32_t k = 0; k < 26u; k++) CHECK(skel_simple(1u << k), "one neighbour: a line end is simple");
    std::printf("simple: %llu masks tested%s, %llu simple\n", (unsigned long long)tested, all ? " (all 2^26)" : "", (unsigned long long)simple);
}

static void check_bit_order_and_subfields() {
    uint32_t seen = 0u;
    for (uint32_t k = 0; k < kSkelBits; k++) {
        const uint32_t o = skel_mask_offset(k);
        CHECK(o < kLabelOffsets && o != kLabelCentre && (k == 0u || o > skel_mask_offset(k - 1u)), "bit %u: offset %u", k, o);
        CHECK(skel_expand(1u << k) == 1u << o && skel_compress(1u << o) == 1u << k, "bit %u: the two forms", k);
        int dx, dy, dz;
        label_offset(o, dx, dy, dz);
        CHECK(dx == (int)(o % 3u) - 1 && dy == (int)(o / 3u % 3u) - 1 && dz == (int)(o / 9u) - 1 && (dx || dy || dz), "bit %u: label_offset", k);
        seen |= 1u << o;
        // a step along an axis is the shift the test uses
        const uint32_t bit = 1u << o;
        const uint32_t want_x = (dx < 1 ? bit << 1 : 0u) | (dx > -1 ? bit >> 1 : 0u);
        const uint32_t want_y = (dy < 1 ? bit << 3 : 0u) | (dy > -1 ? bit >> 3 : 0u);
        const uint32_t want_z = (dz < 1 ? bit << 9 : 0u) | (dz > -1 ? bit >> 9 : 0u);
        CHECK(skel_step_x(bit) == want_x && skel_step_y(bit) == want_y && skel_step_z(bit) == want_z, "bit %u: the steps", k);
    }
    CHECK(seen == (kSkelAll27 & ~(1u << kLabelCentre)), "the 26 bits are the 26 neighbours");
    CHECK(__builtin_popcount(kSkelFaces) == 6 && __builtin_popcount(kSkelEighteen) == 18 && (kSkelFaces & ~kSkelEighteen) == 0u, "faces and the eighteen");
    // two voxels of one subfield are never 26-adjacent; the eight subfields partition every 2 x 2 x 2 block
    for (uint32_t z = 0; z < 5u; z++)
        for (uint32_t y = 0; y < 5u; y++)
            for (uint32_t x = 0; x < 5u; x++) {
                CHECK(skel_subfield(x, y, z) < 8u, "subfield");
                for (uint32_t o = 0; o < kLabelOffsets; o++) {
                    if (o == kLabelCentre) continue;
                    int dx, dy, dz;
                    label_offset(o, dx, dy, dz);
                    CHECK(skel_subfield(x + 8u + (uint32_t)dx, y + 8u + (uint32_t)dy, z + 8u + (uint32_t)dz) != skel_subfield(x + 8u, y + 8u, z + 8u), "adjacent voxels of one subfield");
                }
            }
    CHECK(skel_class(false, 5u) == VK_SKEL_OFF && skel_class(true, 0u) == VK_SKEL_ISOLATED && skel_class(true, 1u) == VK_SKEL_END && skel_class(true, 2u) == VK_SKEL_REGULAR &&
          skel_class(true, 3u) == VK_SKEL_JUNCTION && skel_class(true, 26u) == VK_SKEL_JUNCTION, "classes");
    CHECK(skel_gone(1u) != skel_gone(2u) && skel_gone(1u) == skel_gone(3u) && skel_gone(1u) > kSkelIn && skel_gone(2u) > kSkelIn && skel_gone(2u) < 256u, "the state byte");
    CHECK(skel_was_in(kSkelIn, 4u) && skel_was_in(skel_gone(4u), 4u) && !skel_was_in(skel_gone(3u), 4u) && !skel_was_in(kSkelOff, 4u) && !skel_in(skel_gone(4u)) && skel_in(kSkelIn), "was in K_i");
}

static void check_tiles() {
    // a tile's voxels of the eight subfields are its voxels, each once
    std::vector<uint32_t> hits(kLabelTileVoxels, 0u);
    for (uint32_t s = 0; s < 8u; s++)
        for (uint32_t j = 0; j < kSkelSubVoxels; j++) {
            uint32_t lx, ly, lz;
            skel_sub_coords(j, s, lx, ly, lz);
            CHECK(lx < kLabelTile.tx && ly < kLabelTile.ty && lz < kLabelTile.tz && skel_subfield(lx, ly, lz) == s, "subfield %u voxel %u", s, j);
            hits[label_local_index(lx, ly, lz)]++;
        }
    for (uint32_t h : hits) CHECK(h == 1u, "every voxel of a tile in one subfield, once");
    CHECK(kSkelPerThread * kLabelThreads == kSkelSubVoxels && kSkelSubVoxels == 512u && kGeoWinX == 34u && kGeoWinY == 18u && kGeoWinZ == 10u, "512 voxels per sub-pass; the window");
    // every voxel lies in exactly one tile; every adjacency across tiles is to a tile among the 27 a deleting tile stamps
    const uint32_t nx = 70u, ny = 35u, nz = 18u;
    const uint32_t ntx = (nx + kLabelTile.tx - 1u) / kLabelTile.tx, nty = (ny + kLabelTile.ty - 1u) / kLabelTile.ty, ntz = (nz + kLabelTile.tz - 1u) / kLabelTile.tz;
    std::vector<uint32_t> owners((size_t)nx * ny * nz, 0u);
    for (uint32_t t = 0; t < ntx * nty * ntz; t++) {
        const uint32_t tx = t % ntx, ty = t / ntx % nty, tz = t / (ntx * nty);
        for (uint32_t e = 0; e < kLabelTileVoxels; e++) {
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            const uint32_t x = tx * kLabelTile.tx + lx, y = ty * kLabelTile.ty + ly, z = tz * kLabelTile.tz + lz;
            if (x >= nx || y >= ny || z >= nz) continue;
            owners[voxel_index(x, y, z, nx, ny)]++;
            CHECK(geo_tile_of(x, y, z, ntx, nty) == t, "the tile of a voxel");
            for (uint32_t o = 0; o < kLabelOffsets; o++) {
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                const int64_t ux = (int64_t)x + dx, uy = (int64_t)y + dy, uz = (int64_t)z + dz;
                if (ux < 0 || uy < 0 || uz < 0 || ux >= (int64_t)nx || uy >= (int64_t)ny || uz >= (int64_t)nz) continue;
                const uint32_t other = geo_tile_of((uint32_t)ux, (uint32_t)uy, (uint32_t)uz, ntx, nty);
                bool stamped = false;
                for (uint32_t k = 0; k < kLabelOffsets; k++) {
                    uint32_t nb;
                    if (((kSkelAllTiles >> k) & 1u) && geo_tile_neighbour(tx, ty, tz, ntx, nty, ntz, k, nb) && nb == other) stamped = true;
                }
                CHECK(stamped, "voxel (%u, %u, %u) offset %u: its neighbour's tile is not stamped", x, y, z, o);
                // the neighbour is a cell of the tile's window
                CHECK(geo_window_index((uint32_t)((int)lx + 1 + dx), (uint32_t)((int)ly + 1 + dy), (uint32_t)((int)lz + 1 + dz)) < kGeoWindow, "the window holds every neighbour");
            }
        }
    }
    for (uint32_t c : owners) CHECK(c == 1u, "every voxel in exactly one tile");
}

// ---- the iterations, as the device runs them ---------------------------------------------------------------------------------------------
struct HostWin {
    static uint32_t load(const uint8_t *p, uint32_t i) { return p[i]; }
};

static void replay_case(uint32_t index) {
    static const uint32_t dims[][3] = {{1, 1, 1}, {40, 1, 1}, {1, 37, 1}, {1, 1, 19}, {33, 17, 9}, {9, 5, 4}, {66, 18, 9}, {35, 33, 17}, {12, 7, 3}};
    const uint32_t *d = dims[rnd_below(sizeof dims / sizeof dims[0])];
    const uint32_t nx = d[0], ny = d[1], nz = d[2];
    const uint64_t n = (uint64_t)nx * ny * nz;
    const uint32_t density = 30u + rnd_below(70u);
    std::vector<uint8_t> vol(n);
    for (auto &v : vol) v = rnd_below(100u) < density ? 255u : 0u;
    uint32_t box[6] = {0u, 0u, 0u, nx, ny, nz};
    if (rnd_below(3u) == 0u)
        for (int c = 0; c < 3; c++) {
            const uint32_t ext = c == 0 ? nx : (c == 1 ? ny : nz);
            box[c] = rnd_below(ext + 1u);
            box[c + 3] = box[c] + rnd_below(ext - box[c] + 1u);
        }
    const int mode = (int)rnd_below(2u);
    const uint32_t max_iterations = rnd_below(3u) == 0u ? 1u + rnd_below(3u) : 0u;

    std::vector<uint8_t> want_cls(n), want_dense(n);
    uint64_t want[21];
    CHECK(skel_restate(vol.data(), nx, ny, nz, 0, 0.5f, INFINITY, mode, max_iterations, 0, 0.0f, 0.0f, box, want_cls.data(), want_dense.data(), want) == 0, "the restatement");

    const uint32_t ntx = (nx + kLabelTile.tx - 1u) / kLabelTile.tx, nty = (ny + kLabelTile.ty - 1u) / kLabelTile.ty, ntz = (nz + kLabelTile.tz - 1u) / kLabelTile.tz, tiles = ntx * nty * ntz;
    const vk_voxel_box B = {box[0], box[1], box[2], box[3], box[4], box[5]};
    std::vector<uint8_t> state(n), before(n);
    std::vector<uint32_t> marks[2] = {std::vector<uint32_t>(tiles, 0u), std::vector<uint32_t>(tiles, 0u)};
    for (uint64_t i = 0; i < n; i++) {  // seed
        uint32_t x, y, z;
        label_coords((uint32_t)i, nx, ny, x, y, z);
        const bool in_s = label_in_box(x, y, z, B) && label_foreground((float)vol[i], 0.5f * 255.0f, INFINITY);
        state[i] = in_s ? (uint8_t)kSkelIn : (uint8_t)kSkelOff;
        if (in_s) marks[1][geo_tile_of(x, y, z, ntx, nty)] = 1u;
    }
    uint32_t iterations = 0u, converged = 0u;
    std::vector<uint32_t> order(tiles), voxels(kSkelSubVoxels);
    std::vector<uint8_t> win(kGeoWindow);
    for (uint32_t it = 1u; max_iterations == 0u || it <= max_iterations; it++) {
        uint64_t deleted = 0;
        for (uint32_t s = 0; s < 8u; s++) {
            before = state;
            for (uint32_t t = 0; t < tiles; t++) order[t] = t;
            shuffle(order);
            for (uint32_t t : order) {
                if (marks[it & 1u][t] != it) continue;
                const uint32_t tx = t % ntx, ty = t / ntx % nty, tz = t / (ntx * nty);
                const uint32_t x0 = tx * kLabelTile.tx, y0 = ty * kLabelTile.ty, z0 = tz * kLabelTile.tz;
                for (uint32_t c = 0; c < kGeoWindow; c++) {
                    uint32_t wx, wy, wz;
                    geo_window_coords(c, wx, wy, wz);
                    const int64_t x = (int64_t)x0 + wx - 1, y = (int64_t)y0 + wy - 1, z = (int64_t)z0 + wz - 1;
                    uint8_t st = (uint8_t)kSkelOff;
                    if (x >= 0 && y >= 0 && z >= 0 && x < (int64_t)nx && y < (int64_t)ny && z < (int64_t)nz) {
                        const uint64_t i = voxel_index((uint32_t)x, (uint32_t)y, (uint32_t)z, nx, ny);
                        const bool own = label_in_tile((int)wx - 1, (int)wy - 1, (int)wz - 1);
                        st = (!own && (rnd() & 1u)) ? before[i] : state[i];  // another tile's byte: of before its owner's store, or of after
                    }
                    win[c] = st;
                }
                for (uint32_t j = 0; j < kSkelSubVoxels; j++) voxels[j] = j;
                shuffle(voxels);
                uint32_t here = 0u;
                for (uint32_t j : voxels) {
                    uint32_t lx, ly, lz;
                    skel_sub_coords(j, s, lx, ly, lz);
                    const uint32_t was = win[geo_window_index(lx + 1u, ly + 1u, lz + 1u)];
                    if (was == kSkelOff) continue;
                    const uint32_t now = skel_visit<HostWin>((const uint8_t *)win.data(), lx + 1u, ly + 1u, lz + 1u, it, mode == VK_SKEL_CURVE);
                    if (now == was) continue;
                    CHECK(x0 + lx < nx && y0 + ly < ny && z0 + lz < nz, "a store outside the volume");
                    state[voxel_index(x0 + lx, y0 + ly, z0 + lz, nx, ny)] = (uint8_t)now;
                    here += now != kSkelOff;
                }
                if (here)
                    for (uint32_t k = 0; k < kLabelOffsets; k++) {
                        uint32_t nb;
                        if (geo_tile_neighbour(tx, ty, tz, ntx, nty, ntz, k, nb)) marks[(it + 1u) & 1u][nb] = it + 1u;
                    }
                deleted += here;
            }
        }
        if (!deleted) { converged = 1u; break; }
        iterations++;
    }
    // classes and totals from the state
    uint64_t got[21] = {};
    for (uint64_t i = 0; i < n; i++) {
        uint32_t x, y, z;
        label_coords((uint32_t)i, nx, ny, x, y, z);
        got[0] += label_in_box(x, y, z, B) && vol[i] != 0u;
        const bool in_k = skel_in(state[i]);
        uint32_t m27 = 0u;
        for (uint32_t o = 0; o < kLabelOffsets && in_k; o++) {
            int dx, dy, dz;
            label_offset(o, dx, dy, dz);
            const int64_t hx = (int64_t)x + dx, hy = (int64_t)y + dy, hz = (int64_t)z + dz;
            if (o == kLabelCentre || hx < 0 || hy < 0 || hz < 0 || hx >= (int64_t)nx || hy >= (int64_t)ny || hz >= (int64_t)nz) continue;
            if (skel_in(state[voxel_index((uint32_t)hx, (uint32_t)hy, (uint32_t)hz, nx, ny)])) m27 |= 1u << o;
        }
        const uint32_t c = skel_class(in_k, skel_popcount(skel_compress(m27)));
        CHECK(c == want_cls[i], "case %u (%u x %u x %u, mode %d, cap %u): class of voxel %llu: %u, the restatement %u", index, nx, ny, nz, mode, max_iterations, (unsigned long long)i, c, want_cls[i]);
        if (!in_k) continue;
        got[1]++; got[1u + c]++;
        for (uint32_t j = 0; j < 13u; j++) got[6u + j] += (m27 >> (14u + j)) & 1u;
    }
    got[19] = iterations; got[20] = converged;
    for (int k = 0; k < 21; k++) CHECK(got[k] == want[k], "case %u: result word %d: %llu, the restatement %llu", index, k, (unsigned long long)got[k], (unsigned long long)want[k]);
}

int main(int argc, char **argv) {
    if (argc < 3) { std::printf("usage: skel_fuzz CASES SEED [all]\n"); return 2; }
    const uint32_t cases = (uint32_t)std::strtoul(argv[1], nullptr, 0);
    g_state = std::strtoull(argv[2], nullptr, 0);
    if (!g_state) g_state = 1;
    const bool all = argc > 3 && std::strcmp(argv[3], "all") == 0;
    build_lists();
    check_validation();
    check_bit_order_and_subfields();
    check_tiles();
    check_simple(all);
    for (uint32_t k = 0; k < cases; k++) replay_case(k);
    std::printf("OK (%u cases)\n", cases);
    return 0;
}
