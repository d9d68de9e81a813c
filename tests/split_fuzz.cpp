// split_fuzz.cpp -- vk_split.hpp on the host, under ASan + UBSan: the request's validation, the fill against the range, the tile and seam
// structure of the label pass with its predicate read from a word array (as the split pass uses it for the markers and the residue), and
// the growth's shared step, split_grow_voxel, in double-buffered rounds.  A stand-alone program:
//     split_fuzz CASES SEED
// Per case, on a random volume of up to a few tiles: (1) the predicate lo <= w[i] <= hi from a random word array; every tile's unions in
// a shuffled order in a 4096-word array like the kernel's LDS; the pairs the seam kernel visits -- checked to be every adjacency between
// two tiles, each exactly once -- united in a shuffled order; every root is then the smallest index of its component of a flood fill.
// (2) a random S and K inside it; rounds of split_grow_voxel over the voxels in a shuffled order, each round from one array into the
// other, until a round labels nothing; g (the round that labelled a voxel) and the anchor are then those of a breadth-first search that
// takes the minimum over the neighbours one step closer, and the rounds are the largest g.  No index leaves its array (the arrays are
// exactly as long as the volume: ASan sees the rest).
#include "vk_split.hpp"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

using namespace vk;

static uint64_t g_state;
static uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static uint64_t t_size;
struct HostParent {
    static uint32_t load(std::atomic<uint32_t> *p, uint32_t i) {
        CHECK(i < t_size, "load of %u in an array of %llu", i, (unsigned long long)t_size);
        return p[i].load(std::memory_order_relaxed);
    }
    static uint32_t fetch_min(std::atomic<uint32_t> *p, uint32_t i, uint32_t v) {
        CHECK(i < t_size, "min at %u in an array of %llu", i, (unsigned long long)t_size);
        uint32_t old = p[i].load(std::memory_order_relaxed);
        while (v < old && !p[i].compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
        return old;
    }
};
struct HostState {
    static uint32_t load(const uint32_t *p, uint32_t i) {
        CHECK(i < t_size, "load of %u in an array of %llu", i, (unsigned long long)t_size);
        return p[i];
    }
};
template <class T>
static void shuffle(std::vector<T> &v) {
    for (size_t k = v.size(); k > 1; k--) std::swap(v[k - 1], v[rnd_below((uint32_t)k)]);
}

struct Dims { uint32_t nx, ny, nz, conn, conn_sum; };
static Dims random_dims() {
    static const uint32_t conns[3] = {6u, 18u, 26u};
    Dims d;
    d.nx = 1u + rnd_below(rnd_below(4) ? 40u : 70u); d.ny = 1u + rnd_below(35u); d.nz = 1u + rnd_below(19u);
    d.conn = conns[rnd_below(3)]; d.conn_sum = label_conn_sum(d.conn);
    return d;
}
// the neighbours of voxel i, by the header's words: max |d_c| = 1 and 1 <= sum |d_c| <= conn_sum, no wrap
static std::vector<uint32_t> neighbours(const Dims &d, uint32_t i) {
    uint32_t x, y, z;
    label_coords(i, d.nx, d.ny, x, y, z);
    std::vector<uint32_t> out;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int s = std::abs(dx) + std::abs(dy) + std::abs(dz);
                const long hx = (long)x + dx, hy = (long)y + dy, hz = (long)z + dz;
                if (s < 1 || s > (int)d.conn_sum || hx < 0 || hy < 0 || hz < 0 || hx >= (long)d.nx || hy >= (long)d.ny || hz >= (long)d.nz) continue;
                out.push_back((uint32_t)voxel_index((uint32_t)hx, (uint32_t)hy, (uint32_t)hz, d.nx, d.ny));
            }
    return out;
}
// the smallest index of each component of `in` (a flood fill in raster order); kLabelBackground elsewhere
static std::vector<uint32_t> fill_first(const Dims &d, const std::vector<uint8_t> &in) {
    std::vector<uint32_t> first(in.size(), kLabelBackground), stack;
    for (uint32_t s = 0; s < in.size(); s++) {
        if (!in[s] || first[s] != kLabelBackground) continue;
        first[s] = s;
        stack.assign(1, s);
        while (!stack.empty()) {
            const uint32_t i = stack.back();
            stack.pop_back();
            for (uint32_t j : neighbours(d, i))
                if (in[j] && first[j] == kLabelBackground) { first[j] = s; stack.push_back(j); }
        }
    }
    return first;
}

// ---- the request ---------------------------------------------------------------------------------------------------------------
static vk_split_request good() {
    vk_split_request r{};
    r.lo = 0.5f; r.hi = INFINITY; r.connectivity = 6u; r.radius = 2.0f;
    r.spacing[0] = r.spacing[1] = r.spacing[2] = 1u;
    return r;
}
static void requests() {
    auto ok = [](const vk_split_request &r) { return split_validate(&r, true, false, 0u, false, false) == nullptr; };
    CHECK(split_validate(nullptr, true, false, 0u, false, false) != nullptr, "a NULL request");
    CHECK(ok(good()), "the good request");
    vk_split_request r = good(); r.lo = NAN; CHECK(!ok(r), "lo NaN");
    r = good(); r.hi = NAN; CHECK(!ok(r), "hi NaN");
    r = good(); r.lo = 0.7f; r.hi = 0.6f; CHECK(!ok(r), "lo > hi");
    r = good(); r.lo = r.hi = 0.6f; CHECK(ok(r), "lo == hi");
    r = good(); r.lo = -INFINITY; CHECK(ok(r), "an open range");
    for (uint32_t c = 0; c < 40u; c++) { r = good(); r.connectivity = c; CHECK(ok(r) == (c == 6u || c == 18u || c == 26u), "connectivity %u", c); }
    for (uint32_t f = 0; f < 64u; f++) { r = good(); r.flags = f; CHECK(ok(r) == (f < 4u), "flags %u", f); }
    r = good(); r.flags = 1u << 31; CHECK(!ok(r), "a high flag");
    r = good(); r.pad = 1u; CHECK(!ok(r), "pad");
    for (int a = 0; a < 3; a++)
        for (uint32_t s : {0u, 1u, 64u, 65u, 0xffffffffu}) { r = good(); r.spacing[a] = s; CHECK(ok(r) == (s >= 1u && s <= 64u), "spacing[%d] = %u", a, s); }
    for (float v : {NAN, INFINITY, -INFINITY, -1.0f, -1e-30f, 65535.5f}) { r = good(); r.radius = v; CHECK(!ok(r), "radius %g", v); }
    for (float v : {0.0f, -0.0f, 1e-30f, 7.5f, 65535.0f}) { r = good(); r.radius = v; CHECK(ok(r), "radius %g", v); }
    for (float v : {NAN, INFINITY, -INFINITY}) { r = good(); r.fill_out = v; CHECK(!ok(r), "fill_out %g", v); }
    r = good();
    CHECK(split_validate(&r, false, true, 0u, false, false) != nullptr && split_validate(&r, false, true, 1u, false, false) == nullptr, "components and their room");
    CHECK(split_validate(&r, false, false, 0u, false, false) != nullptr, "nothing asked for");
    CHECK(split_validate(&r, false, false, 0u, true, false) == nullptr && split_validate(&r, false, false, 0u, false, true) == nullptr, "dense_out alone, result alone");
    r.flags = VK_SPLIT_INSTALL; CHECK(split_validate(&r, false, false, 0u, false, false) == nullptr, "the install alone");
    // R2 + 1 fits in a word for every accepted radius: the markers' predicate is R2 + 1 <= D2 <= 0xffffffff
    CHECK(dist_r2(VK_DIST_MAX_RADIUS) + 1u <= 0xffffffffull && dist_r2(7.5f) == 56u && dist_r2(0.0f) == 0u, "R2");
    // every half's value survives the store rule: split_half_value is the inverse of filter_store_f16 off the NaNs
    for (uint32_t h = 0; h < 65536u; h++) {
        const float v = split_half_value(h);
        if ((h & 0x7fffu) > 0x7c00u) { CHECK(v != v, "half %04x is a NaN", h); continue; }
        if ((h & 0x7fffu) == 0x7c00u) { CHECK(std::isinf(v) && (v < 0) == ((h & 0x8000u) != 0u), "half %04x is an infinity", h); continue; }
        CHECK(filter_store_f16(v) == h, "half %04x -> %g -> %04x", h, v, filter_store_f16(v));
    }
    // the fill against the range, on each format's scale
    CHECK(split_fill_leaves_set(0.0f, VK_FMT_R8_UNORM, 127.5f, INFINITY) && !split_fill_leaves_set(0.5f, VK_FMT_R8_UNORM, 127.5f, INFINITY), "u8: 0 leaves, 0.5 stores 128");
    CHECK(split_fill_leaves_set(0.498f, VK_FMT_R8_UNORM, 127.5f, INFINITY) && !split_fill_leaves_set(9.0f, VK_FMT_R8_UNORM, 127.5f, INFINITY), "u8: 127 leaves, a clamped 255 does not");
    CHECK(split_fill_leaves_set(0.0f, VK_FMT_R16_UNORM, 1.0f, 65535.0f) && !split_fill_leaves_set(-3.0f, VK_FMT_R16_UNORM, 0.0f, 1.0f), "u16: the clamp to 0");
    CHECK(split_fill_leaves_set(-1.0f, VK_FMT_R16_FLOAT, 0.0f, INFINITY) && !split_fill_leaves_set(-0.0f, VK_FMT_R16_FLOAT, 0.0f, INFINITY), "f16: -0 >= 0");
    CHECK(!split_fill_leaves_set(70000.0f, VK_FMT_R16_FLOAT, 1.0f, INFINITY) && split_fill_leaves_set(70000.0f, VK_FMT_R16_FLOAT, 1.0f, 65504.0f), "f16: the overflow to +inf");
    CHECK(!split_fill_leaves_set(3.0f, VK_FMT_R16_FLOAT, -INFINITY, INFINITY), "f16: no finite fill leaves the whole line");
}

// ---- tiles and seams with the predicate from an array ----------------------------------------------------------------------------
static void tiles_and_seams(const Dims &d) {
    const uint32_t n = d.nx * d.ny * d.nz;
    std::vector<uint32_t> w(n);
    const uint32_t span = 1u + rnd_below(6u);
    for (uint32_t &v : w) v = rnd_below(3) ? rnd_below(span) : (rnd_below(2) ? kSplitUnreached : kLabelBackground);
    uint32_t lo = rnd_below(span), hi = lo + rnd_below(span);
    if (rnd_below(4) == 0) lo = hi = kSplitUnreached;                 // the residue's predicate
    if (rnd_below(4) == 0) { lo = 1u + rnd_below(span); hi = 0xffffffffu; }  // the markers': R2 + 1 .. INF
    std::vector<uint8_t> fg(n);
    for (uint32_t i = 0; i < n; i++) fg[i] = w[i] >= lo && w[i] <= hi;

    const FilterGrid G = filter_grid(d.nx, d.ny, d.nz, kLabelTile, 0u);
    std::vector<std::atomic<uint32_t>> parent(n);
    std::vector<std::atomic<uint32_t>> lds(kLabelTileVoxels);
    for (uint64_t tile = 0; tile < G.tiles; tile++) {
        uint32_t x0, y0, z0;
        filter_tile_origin(tile, G.ntx, G.nty, kLabelTile, x0, y0, z0);
        for (uint32_t e = 0; e < kLabelTileVoxels; e++) {
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            const bool in = gx < d.nx && gy < d.ny && gz < d.nz && fg[voxel_index(gx, gy, gz, d.nx, d.ny)];
            lds[e].store(in ? e : kLabelBackground);
        }
        std::vector<std::pair<uint32_t, uint32_t>> pairs;
        for (uint32_t e = 0; e < kLabelTileVoxels; e++) {
            if (lds[e].load() == kLabelBackground) continue;
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            for (uint32_t o = 0; o < kLabelCentre; o++) {
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                if (!label_adjacent(dx, dy, dz, d.conn_sum) || !label_in_tile((int)lx + dx, (int)ly + dy, (int)lz + dz)) continue;
                const uint32_t ne = label_local_index(lx + dx, ly + dy, lz + dz);
                if (lds[ne].load() != kLabelBackground) pairs.push_back({e, ne});
            }
        }
        shuffle(pairs);
        t_size = kLabelTileVoxels;
        for (auto &p : pairs) label_union<HostParent>(lds.data(), p.first, p.second);
        for (uint32_t e = 0; e < kLabelTileVoxels; e++) {
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            if (gx >= d.nx || gy >= d.ny || gz >= d.nz) continue;
            uint32_t root = kLabelBackground;
            if (lds[e].load() != kLabelBackground) {
                uint32_t rx, ry, rz;
                label_local_coords(label_find<HostParent>(lds.data(), e), rx, ry, rz);
                root = (uint32_t)voxel_index(x0 + rx, y0 + ry, z0 + rz, d.nx, d.ny);
            }
            parent[voxel_index(gx, gy, gz, d.nx, d.ny)].store(root);
        }
    }
    // the seam kernel's visits: every adjacency between two tiles, each exactly once
    std::multiset<std::pair<uint32_t, uint32_t>> visited;
    std::vector<std::pair<uint32_t, uint32_t>> unions;
    for (uint64_t tile = 0; tile < G.tiles; tile++) {
        uint32_t x0, y0, z0;
        filter_tile_origin(tile, G.ntx, G.nty, kLabelTile, x0, y0, z0);
        for (uint32_t e = 0; e < kLabelSeamVoxels; e++) {
            uint32_t lx, ly, lz;
            label_seam_voxel(e, lx, ly, lz);
            CHECK(label_in_tile((int)lx, (int)ly, (int)lz) && (lx == 0u || ly == 0u || lz == 0u), "seam voxel %u", e);
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            if (gx >= d.nx || gy >= d.ny || gz >= d.nz) continue;
            const uint32_t i = (uint32_t)voxel_index(gx, gy, gz, d.nx, d.ny);
            for (uint32_t o = 0; o < kLabelOffsets; o++) {
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                if (!label_adjacent(dx, dy, dz, d.conn_sum) || !label_seam_owner(lx, ly, lz, dx, dy, dz)) continue;
                const long hx = (long)gx + dx, hy = (long)gy + dy, hz = (long)gz + dz;
                if (hx < 0 || hy < 0 || hz < 0 || hx >= (long)d.nx || hy >= (long)d.ny || hz >= (long)d.nz) continue;
                const uint32_t j = (uint32_t)voxel_index((uint32_t)hx, (uint32_t)hy, (uint32_t)hz, d.nx, d.ny);
                visited.insert({i < j ? i : j, i < j ? j : i});
                if (fg[i] && fg[j]) unions.push_back({i, j});
            }
        }
    }
    auto tile_of = [&](uint32_t i) {
        uint32_t x, y, z;
        label_coords(i, d.nx, d.ny, x, y, z);
        return (uint64_t)(x / kLabelTile.tx) + G.ntx * ((uint64_t)(y / kLabelTile.ty) + (uint64_t)G.nty * (z / kLabelTile.tz));
    };
    std::multiset<std::pair<uint32_t, uint32_t>> wanted;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t j : neighbours(d, i))
            if (i < j && tile_of(i) != tile_of(j)) wanted.insert({i, j});
    CHECK(visited == wanted, "the seam pairs of %u x %u x %u at connectivity %u: %zu visited, %zu adjacencies between tiles", d.nx, d.ny, d.nz, d.conn, visited.size(), wanted.size());
    shuffle(unions);
    t_size = n;
    for (auto &p : unions) label_union<HostParent>(parent.data(), p.first, p.second);
    const std::vector<uint32_t> first = fill_first(d, fg);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t got = fg[i] ? label_find<HostParent>(parent.data(), i) : parent[i].load();
        CHECK(got == first[i], "voxel %u: root %u, the component's first voxel %u", i, got, first[i]);
    }
}

// ---- the growth ----------------------------------------------------------------------------------------------------------------------
static void growth(const Dims &d) {
    const uint32_t n = d.nx * d.ny * d.nz;
    std::vector<uint8_t> S(n), K(n);
    const uint32_t dense = 2u + rnd_below(8u), seeds = 1u + rnd_below(40u);
    for (uint32_t i = 0; i < n; i++) S[i] = rnd_below(10u) < dense;
    if (rnd_below(8) == 0) std::fill(S.begin(), S.end(), 1);
    if (rnd_below(16) != 0)
        for (uint32_t i = 0; i < n; i++) K[i] = S[i] && rnd_below(seeds + n / 64u) < seeds;  // (one case in 16: K empty)
    const std::vector<uint32_t> marker = fill_first(d, K);
    // the reference: breadth-first, a(v) = min over the neighbours with g = g(v) - 1
    std::vector<uint32_t> g(n, 0xffffffffu), a(n, kLabelBackground), list, next;
    for (uint32_t i = 0; i < n; i++) {
        if (S[i]) a[i] = kSplitUnreached;
        if (K[i]) { g[i] = 0u; a[i] = marker[i]; list.push_back(i); }
    }
    uint32_t want_rounds = 0u;
    for (uint32_t k = 1; !list.empty(); k++) {
        next.clear();
        for (uint32_t u : list)
            for (uint32_t v : neighbours(d, u)) {
                if (!S[v] || g[v] < k) continue;
                if (g[v] == 0xffffffffu) { g[v] = k; a[v] = a[u]; next.push_back(v); }
                else if (a[u] < a[v]) a[v] = a[u];
            }
        if (!next.empty()) want_rounds = k;
        list.swap(next);
    }
    // the library's rounds: from one array into the other, voxels in any order
    std::vector<uint32_t> cur(n), other(n, 0x12345678u), order(n), got_g(n, 0xffffffffu);
    for (uint32_t i = 0; i < n; i++) { cur[i] = K[i] ? marker[i] : (S[i] ? kSplitUnreached : kLabelBackground); order[i] = i; if (K[i]) got_g[i] = 0u; }
    t_size = n;
    uint32_t rounds = 0u;
    for (uint32_t k = 1;; k++) {
        CHECK(k <= n + 1u, "round %u of a volume of %u voxels: every round but the last labels a voxel", k, n);
        shuffle(order);
        uint32_t labelled = 0u;
        for (uint32_t i : order) {
            uint32_t s = cur[i];
            if (s == kSplitUnreached) {
                uint32_t x, y, z;
                label_coords(i, d.nx, d.ny, x, y, z);
                s = split_grow_voxel<HostState>((const uint32_t *)cur.data(), x, y, z, d.nx, d.ny, d.nz, d.conn_sum);
                CHECK(s <= kSplitUnreached, "voxel %u took the state %08x", i, s);
                if (s != kSplitUnreached) { labelled++; got_g[i] = k; }
            }
            other[i] = s;
        }
        cur.swap(other);
        if (!labelled) break;
        rounds = k;
    }
    CHECK(rounds == want_rounds, "%u rounds, the largest g is %u", rounds, want_rounds);
    for (uint32_t i = 0; i < n; i++) CHECK(cur[i] == a[i] && got_g[i] == g[i], "voxel %u: state %08x after round %u, wanted %08x at step %u", i, cur[i], got_g[i], a[i], g[i]);
    // rounds past the fixed point change nothing: a batch may run them
    for (uint32_t i = 0; i < n; i++) {
        uint32_t x, y, z;
        label_coords(i, d.nx, d.ny, x, y, z);
        if (cur[i] == kSplitUnreached) CHECK(split_grow_voxel<HostState>((const uint32_t *)cur.data(), x, y, z, d.nx, d.ny, d.nz, d.conn_sum) == kSplitUnreached, "voxel %u moves after the fixed point", i);
    }
}

int main(int argc, char **argv) {
    const uint32_t cases = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 0) : 100u;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!g_state) g_state = 1;
    requests();
    for (uint32_t k = 0; k < cases; k++) {
        const Dims d = random_dims();
        tiles_and_seams(d);
        growth(d);
    }
    std::printf("OK (%u cases)\n", cases);
    return 0;
}
