// thick_fuzz.cpp -- vk_thick.hpp on the host, under ASan + UBSan: the library's own request validation in its order, the cap on both sides
// of the reach limit, the reach, the window, the box distances and the two skips.  A stand-alone program:
//     thick_fuzz CASES SEED
// Per case a random volume, spacing and pair of tiles: the box-to-box and voxel-to-box distances against the minimum over all voxel
// pairs, and a skipped tile or centre against every voxel it might have reached; and the tiled gather, replayed on the host with the
// library's helpers in a shuffled walk order over a random field of radii, against the scatter by the definition.
#include "vk_thick.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

using namespace vk;

static uint64_t g_state;
static uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static uint64_t d2_of(const uint32_t u[3], const uint32_t v[3], const uint32_t w[3]) {
    uint64_t s = 0;
    for (int c = 0; c < 3; c++) {
        const uint64_t a = (uint64_t)w[c] * (u[c] > v[c] ? u[c] - v[c] : v[c] - u[c]);
        s += a * a;
    }
    return s;
}

static void check_validation() {
    vk_thickness_request ok;
    std::memset(&ok, 0, sizeof ok);
    ok.lo = 0.3f; ok.hi = INFINITY; ok.spacing[0] = ok.spacing[1] = ok.spacing[2] = 1u; ok.max_radius = 16.0f;
    CHECK(thick_validate(&ok, true, false, false) == nullptr && thick_validate(&ok, false, true, false) == nullptr && thick_validate(&ok, false, false, true) == nullptr, "a plain request stands");
    CHECK(thick_validate(nullptr, true, true, true) != nullptr, "NULL");
    // the order: every request below carries every later fault as well, and the first is the one reported
    struct Step { const char *word; void (*change)(vk_thickness_request &); };
    const Step steps[] = {
        {"NaN", [](vk_thickness_request &r) { r.lo = NAN; }},
        {"lo > hi", [](vk_thickness_request &r) { r.lo = 1.0f; r.hi = 0.5f; }},
        {"unknown flag", [](vk_thickness_request &r) { r.flags = 4u; }},
        {"a spacing outside", [](vk_thickness_request &r) { r.spacing[1] = 65u; }},
        {"max_radius is not finite", [](vk_thickness_request &r) { r.max_radius = 0.5f; }},
        {"VK_THICK_MAX_REACH", [](vk_thickness_request &r) { r.max_radius = 33.0f; }},
        {"gain is negative", [](vk_thickness_request &r) { r.gain = -1.0f; }},
        {"fill_out is not finite", [](vk_thickness_request &r) { r.fill_out = NAN; }},
    };
    const size_t n_steps = sizeof steps / sizeof steps[0];
    for (size_t first = 0; first < n_steps; first++) {
        vk_thickness_request r = ok;
        for (size_t k = n_steps; k-- > first;) steps[k].change(r);  // (where two faults share a field the earlier one is written last)
        const char *why = thick_validate(&r, false, false, false);
        CHECK(why && std::strstr(why, steps[first].word), "fault %zu: got \"%s\", expected \"%s\"", first, why ? why : "(accepted)", steps[first].word);
    }
    const char *why = thick_validate(&ok, false, false, false);
    CHECK(why && std::strstr(why, "the result would go nowhere"), "nothing requested comes last");
    vk_thickness_request r = ok;
    r.flags = VK_THICK_INSTALL | VK_THICK_CLIP_BOX;
    CHECK(thick_validate(&r, false, false, false) == nullptr, "INSTALL alone is a request");
    for (int c = 0; c < 3; c++) {
        r = ok; r.spacing[c] = 0u;
        CHECK(thick_validate(&r, true, false, false) != nullptr, "spacing 0");
        r.spacing[c] = 64u;
        CHECK(thick_validate(&r, true, false, false) == nullptr, "spacing 64");
    }
    for (float bad : {NAN, INFINITY, -INFINITY, -1.0f, 0.0f, 0.99f}) {
        r = ok; r.max_radius = bad;
        CHECK(thick_validate(&r, true, false, false) != nullptr, "max_radius %f", bad);
    }
    for (float bad : {NAN, INFINITY, -0.5f}) {
        r = ok; r.gain = bad;
        CHECK(thick_validate(&r, true, false, false) != nullptr, "gain %f", bad);
        r = ok; r.fill_out = bad == -0.5f ? -INFINITY : bad;
        CHECK(thick_validate(&r, true, false, false) != nullptr, "fill_out");
    }
    // C on both sides of the reach limit, at every spacing: max_radius = 32 w stands and gives (32 w)^2, the next float above is refused
    for (uint32_t w = 1; w <= (uint32_t)VK_DIST_MAX_SPACING; w++) {
        r = ok; r.spacing[0] = w; r.spacing[1] = (uint32_t)VK_DIST_MAX_SPACING; r.spacing[2] = w + (w < 64u ? 1u : 0u);
        r.max_radius = 32.0f * (float)w;
        CHECK(thick_validate(&r, true, false, false) == nullptr && thick_cap(r.max_radius) == (uint64_t)(32u * w) * (32u * w) && thick_cap(r.max_radius) <= kThickMaxC, "w %u: at the limit", w);
        CHECK(thick_reach(thick_cap(r.max_radius), w) == 31u && thick_reach(thick_cap(r.max_radius) + 1u, w) == 32u, "w %u: (32 w)^2 is not < C = (32 w)^2: the ball is open", w);
        r.max_radius = std::nextafterf(r.max_radius, INFINITY);
        CHECK(thick_validate(&r, true, false, false) != nullptr, "w %u: above the limit", w);
    }
    CHECK(thick_cap(1.0f) == 1u && thick_cap(1.5f) == 2u && thick_cap(6.0f) == 36u && thick_cap(2048.0f) == kThickMaxC && kThickMaxC == (1ull << 22), "C");
    CHECK(thick_reach(1u, 1u) == 0u && thick_reach(2u, 1u) == 1u && thick_reach(36u, 1u) == 5u && thick_reach(37u, 1u) == 6u && thick_reach(37u, 5u) == 1u && thick_reach(kThickMaxC, 64u) == 31u, "reach");
    CHECK(thick_auto_gain(0u) == 0.0f && thick_auto_gain(4u) == 0.5f && kThickMaxWindow == 9u, "gain, window");
}

struct Volume {
    uint32_t n[3], w[3], nt[3];
    uint32_t voxels() const { return n[0] * n[1] * n[2]; }
    uint32_t index(const uint32_t v[3]) const { return v[0] + n[0] * (v[1] + n[1] * v[2]); }
};
static Volume random_volume(uint32_t most) {
    Volume V;
    for (int c = 0; c < 3; c++) {
        V.n[c] = rnd_below(5) == 0 ? 1u : 1u + rnd_below(most);
        V.w[c] = rnd_below(4) == 0 ? (uint32_t)VK_DIST_MAX_SPACING : 1u + rnd_below(6);
        V.nt[c] = thick_tiles_along(V.n[c]);
    }
    return V;
}
template <class F>
static void for_box(const ThickBox &b, F &&f) {
    uint32_t v[3];
    for (v[2] = b.lo[2]; v[2] <= b.hi[2]; v[2]++)
        for (v[1] = b.lo[1]; v[1] <= b.hi[1]; v[1]++)
            for (v[0] = b.lo[0]; v[0] <= b.hi[0]; v[0]++) f(v);
}

// the two distances are the minima they claim to be, and what the skips drop reaches nothing
static void fuzz_skips() {
    const Volume V = random_volume(27);
    uint32_t a[3], b[3];
    for (int c = 0; c < 3; c++) { a[c] = rnd_below(V.nt[c]); b[c] = rnd_below(V.nt[c]); }
    const ThickBox src = thick_tile_box(a[0], a[1], a[2], V.n[0], V.n[1], V.n[2]), out = thick_tile_box(b[0], b[1], b[2], V.n[0], V.n[1], V.n[2]);
    for (int c = 0; c < 3; c++) CHECK(src.lo[c] <= src.hi[c] && src.hi[c] < V.n[c] && src.hi[c] - src.lo[c] < kThickTile && src.lo[c] == a[c] * kThickTile, "a tile's box");
    uint64_t least = std::numeric_limits<uint64_t>::max();
    for_box(src, [&](const uint32_t u[3]) {
        uint64_t mine = std::numeric_limits<uint64_t>::max();
        for_box(out, [&](const uint32_t v[3]) { mine = std::min(mine, d2_of(u, v, V.w)); });
        CHECK(thick_voxel_box_d2(u[0], u[1], u[2], out, V.w) == mine, "voxel to box");
        least = std::min(least, mine);
    });
    const uint64_t bd = thick_box_box_d2(src, out, V.w);
    CHECK(bd == least && bd == thick_box_box_d2(out, src, V.w), "box to box: %llu, over all pairs %llu", (unsigned long long)bd, (unsigned long long)least);
    // a tile maximum about the box distance, a running minimum about it
    const uint32_t top = (uint32_t)std::min<uint64_t>(kThickMaxC, bd + rnd_below(3) - std::min<uint64_t>(bd, 1u) + (rnd_below(2) ? rnd_below(200) : 0u));
    const uint32_t lowest = rnd_below(3) ? rnd_below(top + 2u) : 0u;
    const bool skipped = thick_tile_skipped(top, bd, lowest);
    for_box(src, [&](const uint32_t u[3]) {
        const uint32_t dc = top ? 1u + rnd_below(top) : 0u;  // any radius the tile may hold
        const bool kept = dc && thick_centre_kept(dc, thick_voxel_box_d2(u[0], u[1], u[2], out, V.w), lowest);
        if (!skipped && kept) return;
        for_box(out, [&](const uint32_t v[3]) {  // dropped: it raises no voxel whose running T2 is >= lowest
            const bool reaches = d2_of(u, v, V.w) < dc;
            CHECK(!reaches || dc <= lowest, "a dropped centre of radius^2 %u reaches a voxel and lies above the running minimum %u", dc, lowest);
        });
    });
    // the window holds every tile a ball of the reach can come from, and no more than kThickMaxWindow
    const uint32_t C = 1u + rnd_below(rnd_below(2) ? 40u : (uint32_t)kThickMaxC);
    for (int c = 0; c < 3; c++) {
        const uint32_t reach = std::min<uint32_t>(thick_reach(C, V.w[c]), VK_THICK_MAX_REACH);
        uint32_t first, last;
        thick_window(b[c], V.nt[c], reach, first, last);
        CHECK(first <= b[c] && b[c] <= last && last < V.nt[c] && last - first + 1u <= kThickMaxWindow, "window");
        for (uint32_t u = 0; u < V.n[c]; u++)
            for (uint32_t v = out.lo[c]; v <= out.hi[c]; v++) {
                const uint64_t g = (uint64_t)V.w[c] * (u > v ? u - v : v - u);
                if (g * g < C) CHECK(u / kThickTile >= first && u / kThickTile <= last, "a centre within reach lies outside the window");
            }
    }
}

// the tiled gather as the kernel walks it, in a shuffled order, against the scatter by the definition
static void fuzz_gather() {
    const Volume V = random_volume(19);
    const uint32_t n = V.voxels();
    const uint32_t wmin = thick_min_spacing(V.w);
    const uint32_t C = (uint32_t)thick_cap((float)wmin * (1.0f + (float)rnd_below(rnd_below(3) ? 6u : 32u)));
    std::vector<uint32_t> dc(n, 0u);
    const uint32_t density = 1u + rnd_below(10);
    for (uint32_t i = 0; i < n; i++)
        if (rnd_below(10) < density) dc[i] = rnd_below(4) == 0 ? C : 1u + rnd_below(C);  // any field of radii will do: the rule does not ask where Dc comes from
    std::vector<uint32_t> want(n, 0u), got(n, 0xdeadbeefu);
    {
        uint32_t u[3], v[3];
        for (u[2] = 0; u[2] < V.n[2]; u[2]++) for (u[1] = 0; u[1] < V.n[1]; u[1]++) for (u[0] = 0; u[0] < V.n[0]; u[0]++) {
            const uint32_t r = dc[V.index(u)];
            if (!r) continue;
            for (v[2] = 0; v[2] < V.n[2]; v[2]++) for (v[1] = 0; v[1] < V.n[1]; v[1]++) for (v[0] = 0; v[0] < V.n[0]; v[0]++) {
                const uint32_t iv = V.index(v);
                if (dc[iv] && d2_of(u, v, V.w) < r && want[iv] < r) want[iv] = r;
            }
        }
    }
    uint32_t reach[3];
    for (int c = 0; c < 3; c++) { reach[c] = thick_reach(C, V.w[c]); CHECK(reach[c] <= (uint32_t)VK_THICK_MAX_REACH, "reach"); }
    const uint32_t tiles = V.nt[0] * V.nt[1] * V.nt[2];
    std::vector<uint32_t> tile_max(tiles, 0u);
    for (uint32_t t = 0; t < tiles; t++) {
        uint32_t tx, ty, tz;
        tile_coords(t, V.nt[0], V.nt[1], tx, ty, tz);
        CHECK(thick_tile_index(tx, ty, tz, V.nt[0], V.nt[1]) == t, "tile numbering");
        for_box(thick_tile_box(tx, ty, tz, V.n[0], V.n[1], V.n[2]), [&](const uint32_t v[3]) { tile_max[t] = std::max(tile_max[t], dc[V.index(v)]); });
    }
    uint64_t written = 0;
    for (uint32_t t = 0; t < tiles; t++) {
        uint32_t tx, ty, tz;
        tile_coords(t, V.nt[0], V.nt[1], tx, ty, tz);
        const ThickBox out = thick_tile_box(tx, ty, tz, V.n[0], V.n[1], V.n[2]);
        std::vector<uint32_t> mine;  // the tile's voxels
        for_box(out, [&](const uint32_t v[3]) { mine.push_back(V.index(v)); });
        std::vector<uint32_t> best(mine.size());
        for (size_t k = 0; k < mine.size(); k++) best[k] = dc[mine[k]];
        auto low = [&] {
            uint32_t l = 0xffffffffu;
            for (size_t k = 0; k < mine.size(); k++)
                if (dc[mine[k]]) l = std::min(l, best[k]);
            return l;
        };
        uint32_t lowest = low();
        if (lowest != 0xffffffffu && lowest < C) {
            uint32_t f[3], g[3];
            thick_window(tx, V.nt[0], reach[0], f[0], g[0]);
            thick_window(ty, V.nt[1], reach[1], f[1], g[1]);
            thick_window(tz, V.nt[2], reach[2], f[2], g[2]);
            std::vector<uint32_t> walk;
            for (uint32_t z = f[2]; z <= g[2]; z++) for (uint32_t y = f[1]; y <= g[1]; y++) for (uint32_t x = f[0]; x <= g[0]; x++) walk.push_back(thick_tile_index(x, y, z, V.nt[0], V.nt[1]));
            for (size_t k = walk.size(); k > 1; k--) std::swap(walk[k - 1], walk[rnd_below((uint32_t)k)]);
            for (uint32_t s : walk) {
                if (lowest >= C) break;
                uint32_t sx, sy, sz;
                tile_coords(s, V.nt[0], V.nt[1], sx, sy, sz);
                const ThickBox src = thick_tile_box(sx, sy, sz, V.n[0], V.n[1], V.n[2]);
                if (thick_tile_skipped(tile_max[s], thick_box_box_d2(src, out, V.w), lowest)) continue;
                struct Entry { int32_t p[3]; uint32_t dc; };
                std::vector<Entry> list;
                for_box(src, [&](const uint32_t u[3]) {
                    const uint32_t r = dc[V.index(u)];
                    if (r && thick_centre_kept(r, thick_voxel_box_d2(u[0], u[1], u[2], out, V.w), lowest))
                        list.push_back(Entry{{(int32_t)(V.w[0] * u[0]), (int32_t)(V.w[1] * u[1]), (int32_t)(V.w[2] * u[2])}, r});
                });
                CHECK(list.size() <= kThickTileVoxels, "the list");
                size_t k = 0;
                for_box(out, [&](const uint32_t v[3]) {
                    for (const Entry &e : list) {
                        const uint32_t d2 = thick_d2(e.p[0], e.p[1], e.p[2], (int32_t)(V.w[0] * v[0]), (int32_t)(V.w[1] * v[1]), (int32_t)(V.w[2] * v[2]));
                        if (d2 < e.dc && e.dc > best[k]) best[k] = e.dc;
                    }
                    k++;
                });
                lowest = low();
            }
        }
        for (size_t k = 0; k < mine.size(); k++) {
            CHECK(got[mine[k]] == 0xdeadbeefu, "a voxel is written twice");
            got[mine[k]] = dc[mine[k]] ? best[k] : 0u;
            written++;
        }
    }
    CHECK(written == n, "every voxel is written once");
    for (uint32_t i = 0; i < n; i++)
        CHECK(got[i] == want[i], "%u x %u x %u spacing %u %u %u C %u: voxel %u: the gather gives %u, the scatter %u", V.n[0], V.n[1], V.n[2], V.w[0], V.w[1], V.w[2], C, i, got[i], want[i]);
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!g_state) g_state = 1;
    check_validation();
    for (int k = 0; k < cases; k++) {
        fuzz_skips();
        if (k % 8 == 0) fuzz_gather();
    }
    std::printf("OK (%d cases)\n", cases);
    return 0;
}
