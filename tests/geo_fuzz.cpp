// geo_fuzz.cpp -- vk_geo.hpp on the host, under ASan + UBSan: the library's own request validation in its order, every step cost
// against the floor of 256 sqrt(q) in long double, the saturating relaxation at and around VK_GEO_FAR, the face predicate, the tile and
// halo arithmetic, and the relax kernel's rounds replayed on the host.  A stand-alone program:
//     geo_fuzz CASES SEED
// Per case a random volume, set, spacing, connectivity and source set: rounds over an active-tile set as the device runs them -- tiles
// in a shuffled order, voxels in a shuffled order, halo words taken at random from the state of before the round or of now (the stale
// reads the device may see) -- to the fixed point, against Dijkstra's algorithm.
#include "vk_geo.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <vector>

using namespace vk;

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
    vk_geodesic_request ok;
    std::memset(&ok, 0, sizeof ok);
    ok.lo = 0.3f; ok.hi = INFINITY; ok.connectivity = 26u; ok.spacing[0] = ok.spacing[1] = ok.spacing[2] = 1u; ok.source_faces = VK_GEO_FACE_X0;
    CHECK(geo_validate(&ok, true, false, false) == nullptr && geo_validate(&ok, false, true, false) == nullptr && geo_validate(&ok, false, false, true) == nullptr, "a plain request stands");
    CHECK(geo_validate(nullptr, true, true, true) != nullptr, "NULL");
    // the order: every request below carries every later fault as well, and the first is the one reported
    struct Step { const char *word; void (*change)(vk_geodesic_request &); };
    const Step steps[] = {
        {"NaN", [](vk_geodesic_request &r) { r.hi = NAN; }},
        {"lo > hi", [](vk_geodesic_request &r) { r.lo = 1.0f; r.hi = 0.5f; }},
        {"connectivity must be", [](vk_geodesic_request &r) { r.connectivity = 8u; }},
        {"unknown flag", [](vk_geodesic_request &r) { r.flags = 4u; }},
        {"pad must be 0", [](vk_geodesic_request &r) { r.pad = 1u; }},
        {"a spacing outside", [](vk_geodesic_request &r) { r.spacing[2] = 65u; }},
        {"a face mask", [](vk_geodesic_request &r) { r.target_faces = 64u; }},
        {"n_seeds above", [](vk_geodesic_request &r) { r.n_seeds = 17u; }},
        {"gain is negative", [](vk_geodesic_request &r) { r.gain = -1.0f; }},
        {"fill_out or fill_unreached", [](vk_geodesic_request &r) { r.fill_unreached = NAN; }},
    };
    const size_t n_steps = sizeof steps / sizeof steps[0];
    for (size_t first = 0; first < n_steps; first++) {
        vk_geodesic_request r = ok;
        for (size_t k = n_steps; k-- > first;) steps[k].change(r);
        const char *why = geo_validate(&r, false, false, false);
        CHECK(why && std::strstr(why, steps[first].word), "fault %zu: got \"%s\", expected \"%s\"", first, why ? why : "(accepted)", steps[first].word);
    }
    {   // no source stands between the seed count and the gain
        vk_geodesic_request r = ok;
        r.source_faces = 0u; r.gain = -1.0f; r.fill_out = INFINITY;
        const char *why = geo_validate(&r, false, false, false);
        CHECK(why && std::strstr(why, "no source"), "no source: got \"%s\"", why ? why : "(accepted)");
        r.n_seeds = 1u;
        why = geo_validate(&r, false, false, false);
        CHECK(why && std::strstr(why, "gain is negative"), "a seed is a source: got \"%s\"", why ? why : "(accepted)");
        r = ok; r.source_faces = 64u | 1u;
        why = geo_validate(&r, true, false, false);
        CHECK(why && std::strstr(why, "a face mask"), "source mask");
    }
    const char *why = geo_validate(&ok, false, false, false);
    CHECK(why && std::strstr(why, "the result would go nowhere"), "nothing requested comes last");
    vk_geodesic_request r = ok;
    r.flags = VK_GEO_INSTALL | VK_GEO_CLIP_BOX;
    CHECK(geo_validate(&r, false, false, false) == nullptr, "INSTALL alone is a request");
    for (uint32_t conn : {0u, 1u, 4u, 7u, 27u, 0xffffffffu}) { r = ok; r.connectivity = conn; CHECK(geo_validate(&r, true, false, false) != nullptr, "connectivity %u", conn); }
    for (uint32_t conn : {6u, 18u, 26u}) { r = ok; r.connectivity = conn; CHECK(geo_validate(&r, true, false, false) == nullptr, "connectivity %u", conn); }
    for (int c = 0; c < 3; c++) {
        r = ok; r.spacing[c] = 0u;
        CHECK(geo_validate(&r, true, false, false) != nullptr, "spacing 0");
        r.spacing[c] = 64u;
        CHECK(geo_validate(&r, true, false, false) == nullptr, "spacing 64");
    }
    for (float bad : {NAN, INFINITY, -0.5f}) {
        r = ok; r.gain = bad;
        CHECK(geo_validate(&r, true, false, false) != nullptr, "gain %f", bad);
        r = ok; r.fill_out = bad == -0.5f ? -INFINITY : bad;
        CHECK(geo_validate(&r, true, false, false) != nullptr, "fill_out");
        r = ok; r.fill_unreached = bad == -0.5f ? -INFINITY : bad;
        CHECK(geo_validate(&r, true, false, false) != nullptr, "fill_unreached");
    }
    r = ok; r.source_faces = 63u; r.target_faces = 63u; r.n_seeds = 16u;
    CHECK(geo_validate(&r, true, false, false) == nullptr, "every face, every seed");
    for (uint32_t s = 0; s < 16u; s++) { r.seeds[s][0] = 4u; r.seeds[s][1] = 5u; r.seeds[s][2] = 6u; }
    CHECK(geo_seeds_inside(&r, 5u, 6u, 7u) && !geo_seeds_inside(&r, 4u, 6u, 7u) && !geo_seeds_inside(&r, 5u, 5u, 7u) && !geo_seeds_inside(&r, 5u, 6u, 6u), "seeds against the volume");
    r.n_seeds = 0u;
    CHECK(geo_seeds_inside(&r, 1u, 1u, 1u), "no seed in use");
    CHECK(geo_auto_gain(0u) == 0.0f && geo_auto_gain(4u) == 0.25f && geo_auto_gain(0xFFFFFFFEu) == 1.0f / 4294967296.0f, "gain");
}

// every spacing, every offset: w against floor(256 sqrt(q)) in long double, and w as a non-decreasing function of q
static void check_weights() {
    std::vector<uint32_t> by_q(12289u, 0xffffffffu);
    for (uint32_t sx = 1; sx <= 64u; sx++)
        for (uint32_t sy = 1; sy <= 64u; sy++)
            for (uint32_t sz = 1; sz <= 64u; sz++) {
                const uint32_t sp[3] = {sx, sy, sz};
                for (uint32_t o = 0; o < kLabelOffsets; o++) {
                    if (o == kLabelCentre) continue;
                    int dx, dy, dz;
                    label_offset(o, dx, dy, dz);
                    const uint32_t q = (dx ? sx * sx : 0u) + (dy ? sy * sy : 0u) + (dz ? sz * sz : 0u);
                    const uint32_t w = geo_weight(sp, dx, dy, dz);
                    if (by_q[q] != 0xffffffffu) { CHECK(by_q[q] == w, "w depends on q alone: q %u", q); continue; }
                    by_q[q] = w;
                    const long double root = floorl(256.0L * sqrtl((long double)q));
                    CHECK((long double)w == root && (uint64_t)w * w <= (uint64_t)q << 16 && (uint64_t)(w + 1u) * (w + 1u) > (uint64_t)q << 16, "q %u: w %u, floor(256 sqrt q) %Lf", q, w, root);
                }
            }
    uint32_t last = 0u;
    for (uint32_t q = 1; q <= 12288u; q++) {
        if (by_q[q] == 0xffffffffu) continue;
        CHECK(by_q[q] >= last && by_q[q] >= 256u && by_q[q] < (1u << 15), "monotone in q: q %u", q);
        last = by_q[q];
    }
    CHECK(by_q[1] == 256u && by_q[2] == 362u && by_q[3] == 443u && by_q[4096] == 16384u && by_q[8192] == 23170u && by_q[12288] == 28377u, "the header's costs");
    const uint32_t sp[3] = {1u, 2u, 3u};
    std::vector<uint32_t> seen;
    for (uint32_t o = 0; o < kLabelOffsets; o++) {
        int dx, dy, dz;
        label_offset(o, dx, dy, dz);
        if (o != kLabelCentre) seen.push_back(geo_weight(sp, dx, dy, dz));
    }
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    CHECK((seen == std::vector<uint32_t>{256u, 512u, 572u, 768u, 809u, 923u, 957u}), "the costs at spacing (1, 2, 3)");
    for (uint32_t conn_sum = 1; conn_sum <= 3u; conn_sum++) {
        const GeoWeights W = geo_weights(sp, conn_sum);
        uint32_t used = 0u;
        for (uint32_t o = 0; o < kLabelOffsets; o++) used += W.w[o] != 0u;
        CHECK(used == (conn_sum == 1u ? 6u : (conn_sum == 2u ? 18u : 26u)) && W.w[kLabelCentre] == 0u, "the table of connectivity %u", conn_sum);
    }
}

static void check_relax() {
    CHECK(geo_relax(0u, 256u) == 256u && geo_relax(kGeoFar, 1u) == kGeoFar && geo_relax(kGeoFar, 28377u) == kGeoFar, "plain and saturated");
    for (uint32_t w : {1u, 256u, 362u, 28377u, 32767u})
        for (uint32_t back = 0; back < 70000u; back += 1u + rnd_below(7)) {
            const uint32_t a = kGeoFar - back, s = geo_relax(a, w);
            const uint64_t exact = (uint64_t)a + w;
            CHECK(s != kGeoInf && s >= a && s == (exact < kGeoFar ? (uint32_t)exact : kGeoFar), "a %u w %u: %u", a, w, s);
        }
    for (int k = 0; k < 100000; k++) {  // monotone, and commutes with min
        const uint32_t a = rnd_below(2) ? kGeoFar - rnd_below(100000u) : (uint32_t)rnd() % kGeoFar, b = rnd_below(2) ? kGeoFar - rnd_below(100000u) : (uint32_t)rnd() % kGeoFar;
        const uint32_t w = 1u + rnd_below(32767u);
        CHECK((a <= b) == (geo_relax(a, w) <= geo_relax(b, w)) || geo_relax(a, w) == geo_relax(b, w), "monotone");
        CHECK(geo_relax(std::min(a, b), w) == std::min(geo_relax(a, w), geo_relax(b, w)), "commutes with min");
    }
}

static void check_faces() {
    for (int k = 0; k < 2000; k++) {
        uint32_t n[3], lo[3], hi[3];
        for (int c = 0; c < 3; c++) {
            n[c] = 1u + rnd_below(9);
            lo[c] = rnd_below(3) == 0 ? 0u : rnd_below(n[c]);
            hi[c] = rnd_below(3) == 0 ? n[c] : lo[c] + 1u + rnd_below(n[c] - lo[c]);  // not empty
        }
        const vk_voxel_box b{lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
        for (uint32_t z = lo[2]; z < hi[2]; z++)
            for (uint32_t y = lo[1]; y < hi[1]; y++)
                for (uint32_t x = lo[0]; x < hi[0]; x++) {
                    const bool on[6] = {x == lo[0], x == hi[0] - 1u, y == lo[1], y == hi[1] - 1u, z == lo[2], z == hi[2] - 1u};
                    for (uint32_t mask = 0; mask < 64u; mask++) {
                        bool want = false;
                        for (int f = 0; f < 6; f++) want = want || (((mask >> f) & 1u) && on[f]);
                        CHECK(geo_on_faces(x, y, z, b, mask) == want, "(%u %u %u) mask %u", x, y, z, mask);
                    }
                }
    }
}

struct Volume {
    uint32_t n[3], nt[3], sp[3], conn_sum;
    uint32_t voxels() const { return n[0] * n[1] * n[2]; }
    uint32_t tiles() const { return nt[0] * nt[1] * nt[2]; }
};
static Volume random_volume() {
    Volume V;
    const uint32_t most[3] = {70u, 34u, 18u}, tile[3] = {kLabelTile.tx, kLabelTile.ty, kLabelTile.tz};
    for (int c = 0; c < 3; c++) {
        V.n[c] = rnd_below(5) == 0 ? 1u : (rnd_below(5) == 0 ? tile[c] * (1u + rnd_below(2)) : 1u + rnd_below(most[c]));
        V.nt[c] = (V.n[c] + tile[c] - 1u) / tile[c];
        V.sp[c] = rnd_below(4) == 0 ? (uint32_t)VK_DIST_MAX_SPACING : 1u + rnd_below(8);
    }
    while (V.voxels() > 12000u) { V.n[0] = (V.n[0] + 1u) / 2u; V.nt[0] = (V.n[0] + tile[0] - 1u) / tile[0]; }
    V.conn_sum = 1u + rnd_below(3);
    return V;
}

// every voxel lies in exactly one tile; every adjacency that crosses tiles wakes the tile of the other end, and nothing else is woken
static void check_tiles(const Volume &V) {
    std::vector<uint32_t> owner(V.voxels(), 0u);
    for (uint32_t t = 0; t < V.tiles(); t++) {
        uint32_t x0, y0, z0;
        filter_tile_origin(t, V.nt[0], V.nt[1], kLabelTile, x0, y0, z0);
        for (uint32_t e = 0; e < kLabelTileVoxels; e++) {
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            const uint32_t x = x0 + lx, y = y0 + ly, z = z0 + lz;
            if (x >= V.n[0] || y >= V.n[1] || z >= V.n[2]) continue;
            owner[voxel_index(x, y, z, V.n[0], V.n[1])]++;
            CHECK(geo_tile_of(x, y, z, V.nt[0], V.nt[1]) == t, "the tile of a voxel");
            const uint32_t c = geo_window_index(lx + 1u, ly + 1u, lz + 1u);
            uint32_t wx, wy, wz;
            geo_window_coords(c, wx, wy, wz);
            CHECK(c < kGeoWindow && wx == lx + 1u && wy == ly + 1u && wz == lz + 1u, "the window's index and back");
            const uint32_t mask = geo_wake_mask(lx, ly, lz, V.conn_sum);
            uint32_t needed = 0u;
            for (uint32_t o = 0; o < kLabelOffsets; o++) {
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                if (!label_adjacent(dx, dy, dz, V.conn_sum)) continue;
                const int64_t ux = (int64_t)x + dx, uy = (int64_t)y + dy, uz = (int64_t)z + dz;
                if (ux < 0 || uy < 0 || uz < 0 || ux >= (int64_t)V.n[0] || uy >= (int64_t)V.n[1] || uz >= (int64_t)V.n[2]) continue;
                const uint32_t other = geo_tile_of((uint32_t)ux, (uint32_t)uy, (uint32_t)uz, V.nt[0], V.nt[1]);
                if (other == t) continue;
                bool found = false;
                for (uint32_t k = 0; k < kLabelOffsets; k++) {
                    uint32_t nb;
                    if (((mask >> k) & 1u) && geo_tile_neighbour(t % V.nt[0], t / V.nt[0] % V.nt[1], t / (V.nt[0] * V.nt[1]), V.nt[0], V.nt[1], V.nt[2], k, nb) && nb == other) { found = true; needed |= 1u << k; }
                }
                CHECK(found, "voxel (%u %u %u) offset %u: tile %u is not woken", x, y, z, o, other);
            }
            CHECK(!((mask >> kLabelCentre) & 1u), "a tile does not wake itself");
            // a woken tile that exists holds a voxel adjacent to this one, unless the volume ends inside this tile before the voxel's far side
            for (uint32_t k = 0; k < kLabelOffsets; k++) {
                uint32_t nb;
                if (!((mask >> k) & 1u) || ((needed >> k) & 1u)) continue;
                CHECK(!geo_tile_neighbour(t % V.nt[0], t / V.nt[0] % V.nt[1], t / (V.nt[0] * V.nt[1]), V.nt[0], V.nt[1], V.nt[2], k, nb), "voxel (%u %u %u): direction %u is woken for nothing", x, y, z, k);
            }
        }
    }
    for (uint32_t o : owner) CHECK(o == 1u, "every voxel in exactly one tile");
    CHECK(kGeoWindow == 34u * 18u * 10u && kGeoHalo == kGeoWindow - 4096u && kGeoWinPerThread * kLabelThreads >= kGeoWindow, "the window");
}

struct HostLoad {
    static uint32_t load(const uint32_t *p, uint32_t i) { return p[i]; }
};

static std::vector<uint32_t> dijkstra(const Volume &V, const std::vector<uint8_t> &s, const std::vector<uint8_t> &a) {
    std::vector<uint32_t> g(V.voxels(), kGeoInf);
    typedef std::pair<uint32_t, uint32_t> Entry;
    std::priority_queue<Entry, std::vector<Entry>, std::greater<Entry>> heap;
    for (uint32_t i = 0; i < V.voxels(); i++)
        if (a[i]) { g[i] = 0u; heap.push(Entry(0u, i)); }
    while (!heap.empty()) {
        const Entry e = heap.top();
        heap.pop();
        if (e.first != g[e.second]) continue;
        uint32_t x, y, z;
        label_coords(e.second, V.n[0], V.n[1], x, y, z);
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const uint32_t steps = (uint32_t)(std::abs(dx) + std::abs(dy) + std::abs(dz));
                    if (steps < 1u || steps > V.conn_sum) continue;
                    const int64_t ux = (int64_t)x + dx, uy = (int64_t)y + dy, uz = (int64_t)z + dz;
                    if (ux < 0 || uy < 0 || uz < 0 || ux >= (int64_t)V.n[0] || uy >= (int64_t)V.n[1] || uz >= (int64_t)V.n[2]) continue;
                    const uint32_t iu = (uint32_t)voxel_index((uint32_t)ux, (uint32_t)uy, (uint32_t)uz, V.n[0], V.n[1]);
                    if (!s[iu]) continue;
                    const long double ex = (long double)V.sp[0] * dx, ey = (long double)V.sp[1] * dy, ez = (long double)V.sp[2] * dz;
                    const long double q = ex * ex + ey * ey + ez * ez;
                    const uint64_t sum = (uint64_t)e.first + (uint64_t)floorl(256.0L * sqrtl(q));
                    const uint32_t cand = sum < kGeoFar ? (uint32_t)sum : kGeoFar;
                    if (cand < g[iu]) { g[iu] = cand; heap.push(Entry(cand, iu)); }
                }
    }
    return g;
}

// the relax kernel's rounds on the host; base: what the sources start from (0, or a value near VK_GEO_FAR so that the sums saturate)
static void check_rounds(const Volume &V, uint32_t base) {
    const uint32_t n = V.voxels();
    std::vector<uint8_t> s(n), a(n, 0u);
    const uint32_t density = 30u + rnd_below(70);
    for (uint32_t i = 0; i < n; i++) s[i] = rnd_below(100) < density;
    const uint32_t n_src = 1u + rnd_below(4);
    for (uint32_t k = 0; k < n_src; k++) { const uint32_t i = rnd_below(n); a[i] = s[i]; }
    if (rnd_below(2))
        for (uint32_t i = 0; i < n; i++) { uint32_t x, y, z; label_coords(i, V.n[0], V.n[1], x, y, z); if (x == 0u && s[i]) a[i] = 1u; }
    std::vector<uint32_t> want = dijkstra(V, s, a);
    if (base)
        for (uint32_t &g : want) if (g != kGeoInf) g = (uint64_t)base + g < kGeoFar ? base + g : kGeoFar;  // saturating steps compose: min(min(b + w1, FAR) + w2, FAR) = min(b + w1 + w2, FAR)
    const GeoWeights W = geo_weights(V.sp, V.conn_sum);

    std::vector<uint32_t> state(n, kGeoInf), marks[2] = {std::vector<uint32_t>(V.tiles(), 0u), std::vector<uint32_t>(V.tiles(), 0u)};
    for (uint32_t i = 0; i < n; i++) {
        if (!a[i]) continue;
        state[i] = base;
        uint32_t x, y, z;
        label_coords(i, V.n[0], V.n[1], x, y, z);
        const uint32_t t = geo_tile_of(x, y, z, V.nt[0], V.nt[1]);
        marks[1][t] = 1u;
        const uint32_t mask = geo_wake_mask(x % kLabelTile.tx, y % kLabelTile.ty, z % kLabelTile.tz, V.conn_sum);
        for (uint32_t k = 0; k < kLabelOffsets; k++) {
            uint32_t nb;
            if (((mask >> k) & 1u) && geo_tile_neighbour(t % V.nt[0], t / V.nt[0] % V.nt[1], t / (V.nt[0] * V.nt[1]), V.nt[0], V.nt[1], V.nt[2], k, nb)) marks[1][nb] = 1u;
        }
    }
    std::vector<uint32_t> win(kGeoWindow), order, voxels;
    for (uint32_t round = 1;; round++) {
        CHECK(round < 100000u, "the rounds end");
        const std::vector<uint32_t> before = state;  // what a reader may still see of a word its owner lowers in this round
        std::vector<uint32_t> &cur = marks[round & 1u], &next = marks[(round + 1u) & 1u];
        order.clear();
        for (uint32_t t = 0; t < V.tiles(); t++) if (cur[t] == round) order.push_back(t);
        shuffle(order);
        uint32_t woken = 0u;
        for (uint32_t t : order) {
            uint32_t x0, y0, z0;
            filter_tile_origin(t, V.nt[0], V.nt[1], kLabelTile, x0, y0, z0);
            voxels.clear();
            for (uint32_t c = 0; c < kGeoWindow; c++) {
                uint32_t wx, wy, wz;
                geo_window_coords(c, wx, wy, wz);
                const int64_t x = (int64_t)x0 + wx - 1, y = (int64_t)y0 + wy - 1, z = (int64_t)z0 + wz - 1;
                win[c] = kGeoInf;
                if (x < 0 || y < 0 || z < 0 || x >= (int64_t)V.n[0] || y >= (int64_t)V.n[1] || z >= (int64_t)V.n[2]) continue;
                const uint32_t i = (uint32_t)voxel_index((uint32_t)x, (uint32_t)y, (uint32_t)z, V.n[0], V.n[1]);
                const bool own = wx >= 1u && wy >= 1u && wz >= 1u && wx <= kLabelTile.tx && wy <= kLabelTile.ty && wz <= kLabelTile.tz;
                win[c] = own || rnd_below(2) ? state[i] : before[i];
                if (own && s[i]) voxels.push_back(c);
            }
            std::vector<uint8_t> lowered(kGeoWindow, 0u);
            uint32_t passes = 0u;
            for (bool again = true; again;) {
                again = false;
                CHECK(++passes <= kLabelTileVoxels + 1u, "at most 4097 passes");
                shuffle(voxels);
                for (uint32_t c : voxels) {
                    uint32_t wx, wy, wz;
                    geo_window_coords(c, wx, wy, wz);
                    const uint32_t best = geo_relax_voxel_any<HostLoad>((const uint32_t *)win.data(), wx, wy, wz, kGeoWinX, kGeoWinY, kGeoWinZ, V.conn_sum, W, win[c]);
                    if (best < win[c]) { win[c] = best; lowered[c] = 1u; again = true; }
                }
            }
            uint32_t dirs = 0u;
            for (uint32_t c : voxels) {
                if (!lowered[c]) continue;
                uint32_t wx, wy, wz;
                geo_window_coords(c, wx, wy, wz);
                const uint32_t i = (uint32_t)voxel_index(x0 + wx - 1u, y0 + wy - 1u, z0 + wz - 1u, V.n[0], V.n[1]);
                CHECK(win[c] < state[i] && win[c] != kGeoInf && win[c] >= want[i], "a word only decreases, and never below the fixed point: %u, was %u, fixed point %u (base %u)", win[c], state[i], want[i], base);
                state[i] = win[c];
                dirs |= geo_wake_mask(wx - 1u, wy - 1u, wz - 1u, V.conn_sum);
            }
            for (uint32_t k = 0; k < kLabelOffsets; k++) {
                uint32_t nb;
                if (((dirs >> k) & 1u) && geo_tile_neighbour(t % V.nt[0], t / V.nt[0] % V.nt[1], t / (V.nt[0] * V.nt[1]), V.nt[0], V.nt[1], V.nt[2], k, nb)) { next[nb] = round + 1u; woken++; }
            }
        }
        if (!woken) break;
    }
    for (uint32_t i = 0; i < n; i++) CHECK(state[i] == want[i] && (s[i] || state[i] == kGeoInf), "voxel %u: %u, Dijkstra %u (base %u)", i, state[i], want[i], base);
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 100;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!g_state) g_state = 1;
    check_validation();
    check_weights();
    check_relax();
    check_faces();
    for (int k = 0; k < cases; k++) {
        const Volume V = random_volume();
        if (k % 8 == 0) check_tiles(V);
        check_rounds(V, k % 5 == 4 ? kGeoFar - 2000u - rnd_below(60000u) : 0u);
    }
    std::printf("OK (%d cases)\n", cases);
    return 0;
}
