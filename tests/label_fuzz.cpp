// label_fuzz.cpp -- vk_label.hpp on the host, under ASan + UBSan: the library's own find and union, its tile, seam and chunk arithmetic and
// its selection, with std::atomic standing in for the device atomics, against a flood fill over random volumes.  A stand-alone program:
//     label_fuzz CASES SEED
// Per case: the tile phase (every tile's unions in a shuffled order, in a 4096-word array like the kernel's LDS), the seam phase (the
// pairs the seam kernel visits -- checked to be every adjacency between two tiles, each once -- united in a shuffled order, or by four
// threads that interleave), the flatten, and the renumbering by chunk counts and their scan.  Checked: every root is the smallest index
// of its component, ids are the ranks of the roots, every find and union ends within the bound its comment states, and no index leaves
// its array (the arrays are exactly as long as the volume: ASan sees the rest).
#include "vk_label.hpp"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <thread>
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

static thread_local uint64_t t_loads, t_mins, t_size;
struct HostParent {
    static uint32_t load(std::atomic<uint32_t> *p, uint32_t i) {
        CHECK(i < t_size, "load of %u in an array of %llu", i, (unsigned long long)t_size);
        t_loads++;
        return p[i].load(std::memory_order_relaxed);
    }
    static uint32_t fetch_min(std::atomic<uint32_t> *p, uint32_t i, uint32_t v) {
        CHECK(i < t_size, "min at %u in an array of %llu", i, (unsigned long long)t_size);
        t_mins++;
        uint32_t old = p[i].load(std::memory_order_relaxed);
        while (v < old && !p[i].compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
        return old;
    }
};
static void bounded_union(std::atomic<uint32_t> *p, uint64_t size, uint32_t a, uint32_t b) {
    t_loads = t_mins = 0; t_size = size;
    label_union<HostParent>(p, a, b);
    const uint64_t s = (uint64_t)a + b;
    CHECK(t_mins <= s + 1 && t_loads <= 2 * (s + 1) + s, "union(%u, %u): %llu mins, %llu loads", a, b, (unsigned long long)t_mins, (unsigned long long)t_loads);
}
static uint32_t bounded_find(std::atomic<uint32_t> *p, uint64_t size, uint32_t i) {
    t_loads = 0; t_size = size;
    const uint32_t r = label_find<HostParent>(p, i);
    CHECK(t_loads <= (uint64_t)i + 1 && r <= i, "find(%u): %llu loads, root %u", i, (unsigned long long)t_loads, r);
    return r;
}
template <class T>
static void shuffle(std::vector<T> &v) {
    for (size_t k = v.size(); k > 1; k--) std::swap(v[k - 1], v[rnd_below((uint32_t)k)]);
}

static void one_case(uint32_t index) {
    const uint32_t nx = 1 + rnd_below(index % 4 == 0 ? 70 : 40), ny = 1 + rnd_below(20), nz = 1 + rnd_below(20);
    static const uint32_t kConn[3] = {6u, 18u, 26u}, kDensity[5] = {5u, 31u, 50u, 90u, 100u};
    const uint32_t conn_sum = label_conn_sum(kConn[rnd_below(3)]), density = kDensity[rnd_below(5)];
    const uint64_t n = (uint64_t)nx * ny * nz;
    std::vector<uint8_t> fg(n);
    for (auto &f : fg) f = rnd_below(100) < density;
    auto at = [&](int64_t x, int64_t y, int64_t z) { return (uint32_t)voxel_index((uint32_t)x, (uint32_t)y, (uint32_t)z, nx, ny); };
    auto inside = [&](int64_t x, int64_t y, int64_t z) { return x >= 0 && y >= 0 && z >= 0 && x < nx && y < ny && z < nz; };

    // the reference: a flood fill in raster order; want[i] = the smallest index of i's component
    std::vector<uint32_t> want(n, kLabelBackground), stack;
    for (uint64_t s = 0; s < n; s++) {
        if (!fg[s] || want[s] != kLabelBackground) continue;
        stack.assign(1, (uint32_t)s);
        want[s] = (uint32_t)s;
        while (!stack.empty()) {
            const uint32_t i = stack.back();
            stack.pop_back();
            uint32_t x, y, z;
            label_coords(i, nx, ny, x, y, z);
            CHECK(at(x, y, z) == i, "label_coords(%u)", i);
            for (uint32_t o = 0; o < kLabelOffsets; o++) {
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                if (!label_adjacent(dx, dy, dz, conn_sum) || !inside((int64_t)x + dx, (int64_t)y + dy, (int64_t)z + dz)) continue;
                const uint32_t j = at((int64_t)x + dx, (int64_t)y + dy, (int64_t)z + dz);
                if (fg[j] && want[j] == kLabelBackground) { want[j] = (uint32_t)s; stack.push_back(j); }
            }
        }
    }

    // the tile phase
    const FilterGrid G = filter_grid(nx, ny, nz, kLabelTile, 0u);
    std::vector<std::atomic<uint32_t>> parent(n);
    std::vector<uint8_t> written(n, 0);
    for (uint64_t tile = 0; tile < G.tiles; tile++) {
        uint32_t x0, y0, z0;
        filter_tile_origin(tile, G.ntx, G.nty, kLabelTile, x0, y0, z0);
        std::vector<std::atomic<uint32_t>> lds(kLabelTileVoxels);
        for (uint32_t e = 0; e < kLabelTileVoxels; e++) {
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            CHECK(label_local_index(lx, ly, lz) == e && label_in_tile((int)lx, (int)ly, (int)lz), "local index %u", e);
            const bool f = inside(x0 + lx, y0 + ly, z0 + lz) && fg[at(x0 + lx, y0 + ly, z0 + lz)];
            lds[e].store(f ? e : kLabelBackground);
        }
        std::vector<std::pair<uint32_t, uint32_t>> jobs;
        for (uint32_t e = 0; e < kLabelTileVoxels; e++) {
            if (lds[e].load() == kLabelBackground) continue;
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            for (uint32_t o = 0; o < kLabelCentre; o++) {
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                if (!label_adjacent(dx, dy, dz, conn_sum) || !label_in_tile((int)lx + dx, (int)ly + dy, (int)lz + dz)) continue;
                const uint32_t ne = label_local_index(lx + dx, ly + dy, lz + dz);
                CHECK(ne < e, "an earlier neighbour has a smaller local index");
                if (lds[ne].load() != kLabelBackground) jobs.push_back({e, ne});
            }
        }
        shuffle(jobs);
        for (auto &j : jobs) bounded_union(lds.data(), kLabelTileVoxels, j.first, j.second);
        for (uint32_t e = 0; e < kLabelTileVoxels; e++) {
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            if (!inside(x0 + lx, y0 + ly, z0 + lz)) continue;
            uint32_t root = kLabelBackground;
            if (lds[e].load() != kLabelBackground) {
                uint32_t rx, ry, rz;
                label_local_coords(bounded_find(lds.data(), kLabelTileVoxels, e), rx, ry, rz);
                CHECK(inside(x0 + rx, y0 + ry, z0 + rz), "a tile root outside the volume");
                root = at(x0 + rx, y0 + ry, z0 + rz);
            }
            const uint32_t i = at(x0 + lx, y0 + ly, z0 + lz);
            CHECK(!written[i], "voxel %u written by two tiles", i);
            written[i] = 1;
            CHECK(root == kLabelBackground ? !fg[i] : (fg[i] && root <= i && want[root] == want[i]), "tile root of %u", i);
            parent[i].store(root);
        }
    }
    for (uint64_t i = 0; i < n; i++) CHECK(written[i], "voxel %llu written by no tile", (unsigned long long)i);

    // the seam phase: the pairs the kernel visits ...
    std::vector<std::pair<uint32_t, uint32_t>> jobs;
    std::set<std::pair<uint32_t, uint32_t>> seen;
    for (uint64_t tile = 0; tile < G.tiles; tile++) {
        uint32_t x0, y0, z0;
        filter_tile_origin(tile, G.ntx, G.nty, kLabelTile, x0, y0, z0);
        std::set<uint32_t> faces;
        for (uint32_t e = 0; e < kLabelSeamVoxels; e++) {
            uint32_t lx, ly, lz;
            label_seam_voxel(e, lx, ly, lz);
            CHECK(label_in_tile((int)lx, (int)ly, (int)lz) && (lx == 0 || ly == 0 || lz == 0) && faces.insert(label_local_index(lx, ly, lz)).second, "seam voxel %u", e);
            if (!inside(x0 + lx, y0 + ly, z0 + lz)) continue;
            const uint32_t i = at(x0 + lx, y0 + ly, z0 + lz);
            if (!fg[i]) continue;
            for (uint32_t o = 0; o < kLabelOffsets; o++) {
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                if (!label_adjacent(dx, dy, dz, conn_sum) || !label_seam_owner(lx, ly, lz, dx, dy, dz)) continue;
                const int64_t hx = (int64_t)x0 + lx + dx, hy = (int64_t)y0 + ly + dy, hz = (int64_t)z0 + lz + dz;
                if (!inside(hx, hy, hz)) continue;
                const uint32_t j = at(hx, hy, hz);
                if (!fg[j]) continue;
                CHECK(seen.insert({i < j ? i : j, i < j ? j : i}).second, "the pair (%u, %u) is visited twice", i, j);
                jobs.push_back({i, j});
            }
        }
        CHECK(faces.size() == kLabelSeamVoxels, "the three low faces");
    }
    // ... are every adjacency between two tiles
    uint64_t across = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!fg[i]) continue;
        uint32_t x, y, z;
        label_coords((uint32_t)i, nx, ny, x, y, z);
        for (uint32_t o = 0; o < kLabelCentre; o++) {
            int dx, dy, dz;
            label_offset(o, dx, dy, dz);
            if (!label_adjacent(dx, dy, dz, conn_sum) || !inside((int64_t)x + dx, (int64_t)y + dy, (int64_t)z + dz)) continue;
            const uint32_t j = at((int64_t)x + dx, (int64_t)y + dy, (int64_t)z + dz);
            const bool same_tile = x / kLabelTile.tx == (x + dx) / kLabelTile.tx && y / kLabelTile.ty == (y + dy) / kLabelTile.ty && z / kLabelTile.tz == (z + dz) / kLabelTile.tz;
            if (!fg[j] || same_tile) continue;
            across++;
            CHECK(seen.count({j, (uint32_t)i}), "the pair (%u, %llu) between two tiles is not visited", j, (unsigned long long)i);
        }
    }
    CHECK(across == seen.size(), "%llu pairs between tiles, %zu visited", (unsigned long long)across, seen.size());
    shuffle(jobs);
    if (index % 2 == 0) {
        for (auto &j : jobs) bounded_union(parent.data(), n, j.first, j.second);
    } else {  // four threads that interleave: thread t takes jobs t, t + 4, ...
        std::vector<std::thread> threads;
        for (uint32_t t = 0; t < 4; t++)
            threads.emplace_back([&, t] { for (size_t k = t; k < jobs.size(); k += 4) bounded_union(parent.data(), n, jobs[k].first, jobs[k].second); });
        for (auto &t : threads) t.join();
    }

    // flatten; roots and foreground per chunk
    const uint32_t chunks = label_chunks(n);
    CHECK((uint64_t)chunks * kLabelChunk >= n && (chunks == 0 || (uint64_t)(chunks - 1) * kLabelChunk < n), "label_chunks");
    std::vector<uint32_t> chunk_roots(chunks, 0);
    uint64_t n_fg = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (parent[i].load() == kLabelBackground) { CHECK(!fg[i], "foreground voxel %llu lost", (unsigned long long)i); continue; }
        const uint32_t r = bounded_find(parent.data(), n, (uint32_t)i);
        CHECK(fg[i] && r == want[i], "voxel %llu: root %u, the smallest index of its component is %u", (unsigned long long)i, r, want[i]);
        n_fg++;
        if (r == i) chunk_roots[i / kLabelChunk]++;
        else parent[i].store(r);
    }
    // the scan, and ids by thread order inside a chunk: a thread holds kLabelChunkPerThread consecutive voxels
    std::vector<uint32_t> offset(chunks, 0), labels(n, 0), sizes;
    uint32_t n_comp = 0;
    for (uint32_t c = 0; c < chunks; c++) { offset[c] = n_comp; n_comp += chunk_roots[c]; }
    for (uint32_t c = 0; c < chunks; c++) {
        uint32_t before = 0;
        for (uint32_t t = 0; t < kLabelThreads; t++) {
            const uint64_t i0 = (uint64_t)c * kLabelChunk + (uint64_t)t * kLabelChunkPerThread;
            uint32_t id = offset[c] + before + 1u;
            for (uint32_t k = 0; k < kLabelChunkPerThread; k++)
                if (i0 + k < n && parent[i0 + k].load() == i0 + k) { labels[i0 + k] = id++; before++; }
        }
    }
    uint32_t rank = 0;
    sizes.assign(n_comp, 0);
    for (uint64_t i = 0; i < n; i++) {
        if (!fg[i]) continue;
        if (want[i] == i) CHECK(labels[i] == ++rank, "root %llu takes id %u, its rank is %u", (unsigned long long)i, labels[i], rank);
        sizes[labels[want[i]] - 1]++;
    }
    CHECK(rank == n_comp, "%u roots, %u ids", rank, n_comp);

    // the selection against its words
    vk_label_request r{};
    r.keep = (int32_t)rnd_below(3);
    r.count = r.keep == VK_LABEL_KEEP_ALL ? 0u : 1u + rnd_below(6);
    std::vector<uint8_t> keep;
    uint64_t kept_voxels = 0;
    const uint64_t kept = label_select(r, sizes.data(), n_comp, nullptr, keep, &kept_voxels);
    CHECK(keep.size() == (size_t)n_comp + 1 && keep[0] == 0, "keep bytes");
    uint64_t count = 0, voxels = 0;
    for (uint32_t id = 1; id <= n_comp; id++) {
        bool sel = r.keep == VK_LABEL_KEEP_ALL || (r.keep == VK_LABEL_KEEP_MIN_SIZE && sizes[id - 1] >= r.count);
        if (r.keep == VK_LABEL_KEEP_LARGEST) {  // fewer than `count` come before it in (size descending, id ascending)
            uint64_t ahead = 0;
            for (uint32_t o = 1; o <= n_comp; o++) ahead += sizes[o - 1] > sizes[id - 1] || (sizes[o - 1] == sizes[id - 1] && o < id);
            sel = ahead < r.count;
        }
        CHECK((keep[id] != 0) == sel, "component %u of %u under keep %d count %llu", id, n_comp, r.keep, (unsigned long long)r.count);
        if (sel) { count++; voxels += sizes[id - 1]; }
    }
    CHECK(kept == count && kept_voxels == voxels, "the kept totals");
}

static void requests() {
    vk_label_request r{};
    r.lo = 0.3f; r.hi = INFINITY; r.connectivity = 6;
    CHECK(label_validate(&r, true, false, 0, false, false) == nullptr, "a plain request");
    CHECK(label_validate(nullptr, true, false, 0, false, false) && label_validate(&r, false, false, 0, false, false) && label_validate(&r, false, true, 0, false, false), "NULL, no output, cap 0");
    vk_label_request b = r; b.lo = NAN; CHECK(label_validate(&b, true, false, 0, false, false), "NaN");
    b = r; b.lo = 1.0f; b.hi = 0.5f; CHECK(label_validate(&b, true, false, 0, false, false), "lo > hi");
    b = r; b.fill = INFINITY; CHECK(label_validate(&b, true, false, 0, false, false), "fill");
    b = r; b.connectivity = 8; CHECK(label_validate(&b, true, false, 0, false, false), "connectivity");
    b = r; b.flags = 8; CHECK(label_validate(&b, true, false, 0, false, false), "flag");
    b = r; b.keep = 4; CHECK(label_validate(&b, true, false, 0, false, false), "keep");
    b = r; b.pad = 1; CHECK(label_validate(&b, true, false, 0, false, false), "pad");
    b = r; b.count = 1; CHECK(label_validate(&b, true, false, 0, false, false), "count under KEEP_ALL");
    b = r; b.keep = VK_LABEL_KEEP_LARGEST; CHECK(label_validate(&b, true, false, 0, false, false), "count 0 under KEEP_LARGEST");
    b = r; b.keep = VK_LABEL_KEEP_SEEDS; CHECK(label_validate(&b, true, false, 0, false, false), "no seeds");
    b.n_seeds = 17; CHECK(label_validate(&b, true, false, 0, false, false), "17 seeds");
    b.n_seeds = 2; b.seeds[1][2] = 5; CHECK(!label_validate(&b, true, false, 0, false, false) && label_seeds_inside(&b, 1, 1, 6) && !label_seeds_inside(&b, 1, 1, 5), "seeds");
    CHECK(label_fill_bits(0.5f, VK_FMT_R8_UNORM) == 128u && label_fill_bits(-1.0f, VK_FMT_R16_UNORM) == 0u && label_fill_bits(7.0f, VK_FMT_R16_UNORM) == 65535u && label_fill_bits(1.0f, VK_FMT_R16_FLOAT) == 0x3c00u, "fill");
    // the size limit, just under and just over 2^32 - 2 voxels: 2^32 - 2 = 2 x 2147483647 itself, and the products of valid dims (<= 8192) around it
    CHECK(label_volume_fits(1, 1, 1) && label_volume_fits(8192, 8192, 63) && label_volume_fits(2147483647u, 2, 1) && label_volume_fits(0xfffffffeu, 1, 1), "volumes of up to 2^32 - 2 voxels");
    CHECK(!label_volume_fits(0xffffffffu, 1, 1) && !label_volume_fits(65535, 65537, 1) && !label_volume_fits(65536, 65536, 1) && !label_volume_fits(8192, 8192, 64) && !label_volume_fits(8192, 8192, 8192), "volumes of 2^32 - 1 voxels and more");
    CHECK(label_blocks(0, 0) == 1 && label_blocks(10, 3) == 3 && label_blocks(1ull << 40, 0) == kLabelMaxBlocks, "label_blocks");
}

int main(int argc, char **argv) {
    const uint32_t cases = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 0) : 100u;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!g_state) g_state = 1;
    requests();
    for (uint32_t k = 0; k < cases; k++) one_case(k);
    std::printf("OK (%u cases)\n", cases);
    return 0;
}
