// The host-callable arithmetic of the volume filter pass (vokselis_amd/csrc/vk_filter.hpp) against brute force, as a
// stand-alone program for plain g++ under -fsanitize=address,undefined: over random dimensions up to 8192 and all radii, the tiles cover
// every output voxel exactly once, every halo index of every pass lies inside its LDS extent, the LDS of every tile shape stays within
// 64 KiB, grid and offset arithmetic stays within its types, the clamp, the store rules, the totalOrder key and the selection network
// agree with their definitions, and the request's validation accepts and refuses what the header says.
//
// usage: filter_fuzz CASES SEED
#include "vk_filter.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace vk;

static uint64_t g_state;
static uint64_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            std::printf("FAILED %s: ", #cond);            \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            std::exit(1);                                 \
        }                                                 \
    } while (0)

static uint32_t random_dim() {
    switch (rnd_below(6)) {
        case 0: return 1u + rnd_below(8u);
        case 1: return 1u + rnd_below(80u);
        case 2: return 8192u - rnd_below(40u);
        case 3: return 32u * (1u + rnd_below(8u)) + rnd_below(3u) - 1u;
        default: return 1u + rnd_below(8192u);
    }
}

// one axis: the tiles of `n` voxels of edge `t` cover [0, n) once each; the first and last tile are where filter_grid says
static void check_axis_cover(uint32_t n, uint32_t t, uint32_t nt) {
    CHECK(nt >= 1u && (uint64_t)(nt - 1u) * t < n && (uint64_t)nt * t >= n, "n %u t %u nt %u", n, t, nt);
}

static void check_tiles(uint32_t nx, uint32_t ny, uint32_t nz, FilterTile T, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t max_blocks, uint32_t elem_bytes) {
    CHECK(rx <= T.r && ry <= T.r && rz <= T.r, "radii within the class");
    CHECK(filter_lds_bytes(T, elem_bytes) <= kFilterLdsLimit, "LDS %u", filter_lds_bytes(T, elem_bytes));
    CHECK((filter_pitch_x(T) & 1u) == 1u && filter_pitch_x(T) >= T.tx + 2u * T.r, "pitch");
    CHECK((T.tx * T.ty * T.tz) % kFilterThreads == 0u, "a tile is a multiple of the workgroup");
    const FilterGrid G = filter_grid(nx, ny, nz, T, max_blocks);
    check_axis_cover(nx, T.tx, G.ntx);
    check_axis_cover(ny, T.ty, G.nty);
    check_axis_cover(nz, T.tz, G.ntz);
    CHECK(G.tiles == (uint64_t)G.ntx * G.nty * G.ntz, "tiles");
    CHECK(G.blocks >= 1u && G.blocks <= kFilterMaxBlocks && (uint64_t)G.blocks * kFilterThreads <= (1ull << 32), "blocks %u", G.blocks);
    CHECK(G.blocks <= G.tiles && (!max_blocks || G.blocks <= max_blocks), "blocks within tiles and the cap");
    // a few tiles -- the first, the last, random ones: origin inside the volume, the inverse of the index, every halo element inside LDS
    const uint32_t hx = T.tx + 2u * rx, hy = T.ty + 2u * ry, hz = T.tz + 2u * rz;
    const uint32_t lds = filter_lds_elems(T);
    for (int k = 0; k < 6; k++) {
        const uint64_t i = k == 0 ? 0u : (k == 1 ? G.tiles - 1u : rnd() % G.tiles);
        uint32_t x0, y0, z0;
        filter_tile_origin(i, G.ntx, G.nty, T, x0, y0, z0);
        CHECK(x0 < nx && y0 < ny && z0 < nz && x0 % T.tx == 0u && y0 % T.ty == 0u && z0 % T.tz == 0u, "origin");
        CHECK((uint64_t)(x0 / T.tx) + (uint64_t)G.ntx * ((uint64_t)(y0 / T.ty) + (uint64_t)G.nty * (z0 / T.tz)) == i, "the origin's tile is the tile");
        // the corners of the halo box and of each pass's reads and writes
        const uint32_t far_load = filter_lds_index(T, hx - 1u, hy - 1u, hz - 1u);
        CHECK(far_load < lds, "load %u of %u", far_load, lds);
        CHECK(filter_lds_index(T, (T.tx - 1u) + 2u * rx, hy - 1u, hz - 1u) < lds, "x pass reads");
        CHECK(filter_lds_index(T, (T.tx - 1u) + rx, (T.ty - 1u) + 2u * ry, hz - 1u) < lds, "y pass reads");
        CHECK(filter_lds_index(T, (T.tx - 1u) + rx, (T.ty - 1u) + ry, (T.tz - 1u) + 2u * rz) < lds, "z pass reads");
        // random halo elements: distinct elements have distinct LDS slots (the pitch covers the row), the clamped voxel lies inside the volume
        for (int j = 0; j < 8; j++) {
            const uint32_t lx = rnd_below(hx), ly = rnd_below(hy), lz = rnd_below(hz);
            const uint32_t idx = filter_lds_index(T, lx, ly, lz);
            CHECK(idx < lds, "halo index");
            CHECK(idx % filter_pitch_x(T) == lx && (idx / filter_pitch_x(T)) % filter_rows(T) == ly && idx / (filter_pitch_x(T) * filter_rows(T)) == lz, "the index is invertible");
            const uint32_t gx = filter_clamp((int64_t)x0 + lx - rx, nx), gy = filter_clamp((int64_t)y0 + ly - ry, ny), gz = filter_clamp((int64_t)z0 + lz - rz, nz);
            CHECK(gx < nx && gy < ny && gz < nz, "clamped voxel");
            const uint64_t off = filter_voxel_offset(gx, gy, gz, nx, ny);
            CHECK(off < (uint64_t)nx * ny * nz, "offset");
        }
    }
    // items per thread of each pass cover the pass
    CHECK((uint64_t)filter_per_thread(T.tx * filter_rows(T) * filter_planes(T)) * kFilterThreads >= (uint64_t)T.tx * hy * hz, "x pass items");
    CHECK((uint64_t)filter_per_thread(T.tx * T.ty * filter_planes(T)) * kFilterThreads >= (uint64_t)T.tx * T.ty * hz, "y pass items");
}

// small volumes: every voxel belongs to exactly one tile
static void check_cover_brute(uint32_t nx, uint32_t ny, uint32_t nz, FilterTile T) {
    const FilterGrid G = filter_grid(nx, ny, nz, T, 0u);
    std::vector<uint8_t> seen((size_t)nx * ny * nz, 0);
    for (uint64_t i = 0; i < G.tiles; i++) {
        uint32_t x0, y0, z0;
        filter_tile_origin(i, G.ntx, G.nty, T, x0, y0, z0);
        for (uint32_t e = 0; e < T.tx * T.ty * T.tz; e++) {
            const uint32_t row = e / T.tx, lx = e - row * T.tx, lz = row / T.ty, ly = row - lz * T.ty;
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            if (gx < nx && gy < ny && gz < nz) seen[(size_t)filter_voxel_offset(gx, gy, gz, nx, ny)]++;
        }
    }
    for (size_t i = 0; i < seen.size(); i++) CHECK(seen[i] == 1u, "voxel %zu seen %u times", i, (unsigned)seen[i]);
}

static void check_clamp() {
    const uint32_t n = 1u + rnd_below(8192u);
    const int64_t i = (int64_t)rnd_below(3u * 8192u) - 8192;
    const uint32_t c = filter_clamp(i, n);
    const int64_t want = std::min<int64_t>(std::max<int64_t>(i, 0), (int64_t)n - 1);
    CHECK((int64_t)c == want, "clamp(%" PRId64 ", %u) = %u", i, n, c);
}

static float bits_float(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}
// the value of a half, exactly, as a double
static double half_value(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    const double v = e == 0u ? ldexp((double)m, -24) : ldexp((double)(m | 1024u), (int)e - 25);
    return (h & 0x8000u) ? -v : v;
}
static void check_store_f16() {
    uint32_t b = (uint32_t)rnd();
    if (rnd_below(3u) == 0u) b = (b & 0x807fffffu) | ((100u + rnd_below(45u)) << 23);  // the range of halves, denormals and overflow
    const float v = bits_float(b);
    const uint32_t h = filter_store_f16(v);
    CHECK(h <= 0xffffu, "16 bits");
    if (v != v) { CHECK(h == 0x7e00u, "NaN -> 0x7E00, got %#x", h); return; }
    CHECK((h & 0x7fffu) <= 0x7c00u, "never a NaN from a number");
    CHECK(((h >> 15) & 1u) == (b >> 31), "the sign is kept");
    const double a = fabs((double)v);
    const uint32_t m = h & 0x7fffu;
    if (m == 0x7c00u) { CHECK(a >= 65520.0, "overflow only from 65520 on: %a", (double)v); return; }
    CHECK(a < 65520.0, "65520 and above overflow");
    // the nearest of the neighbouring halves, ties to the even one
    const double got = half_value(m), below = m ? half_value(m - 1u) : -1.0, above = m < 0x7bffu ? half_value(m + 1u) : 65536.0;
    const double err = fabs(got - a);
    CHECK(err <= fabs(below - a) && err <= fabs(above - a), "not the nearest: %a -> %#x", (double)v, h);
    if (err == fabs(below - a) || err == fabs(above - a)) CHECK((m & 1u) == 0u || err == 0.0, "a tie goes to the even half: %a -> %#x", (double)v, h);
}
static void check_store_unorm() {
    const float top = rnd_below(2u) ? 255.0f : 65535.0f;
    float v;
    switch (rnd_below(4u)) {
        case 0: v = (float)rnd_below(70000u) - 2000.0f + 0.5f; break;
        case 1: v = bits_float((uint32_t)rnd()); break;
        default: v = ((float)(rnd() % 20000000ull) - 1000000.0f) / 256.0f; break;
    }
    if (!(fabsf(v) <= 3.0e38f)) return;  // finite by the weight bound
    const uint32_t q = filter_store_unorm(v, top);
    const double c = std::min(std::max((double)v, 0.0), (double)top), fl = floor(c), fr = c - fl;
    const double want = fr < 0.5 ? fl : (fr > 0.5 ? fl + 1.0 : (fmod(fl, 2.0) == 0.0 ? fl : fl + 1.0));
    CHECK((double)q == want, "store(%a, %g) = %u, want %g", (double)v, (double)top, q, want);
}

static void check_keys() {
    const uint32_t a = (uint32_t)rnd() & 0xffffu, b = (uint32_t)rnd() & 0xffffu;
    CHECK(filter_f16_unkey(filter_f16_key(a)) == a, "unkey(key) %#x", a);
    // totalOrder: negatives below positives; among negatives the larger magnitude first; -0 below +0; NaNs at the ends by sign
    const bool an = a & 0x8000u, bn = b & 0x8000u;
    const bool less = an != bn ? an : (an ? (a & 0x7fffu) > (b & 0x7fffu) : (a & 0x7fffu) < (b & 0x7fffu));
    CHECK((filter_f16_key(a) < filter_f16_key(b)) == less, "order of %#x and %#x", a, b);
}

static void check_median() {
    uint32_t v[27], s[27];
    const uint32_t span = rnd_below(3u) == 0u ? 3u : (rnd_below(2u) ? 256u : 65536u);
    for (int i = 0; i < 27; i++) v[i] = s[i] = rnd_below(span);
    std::sort(s, s + 27);
    const uint32_t m = filter_median27(v);
    CHECK(m == s[13], "median %u, want %u", m, s[13]);
}

static struct vk_volume_filter random_request() {
    struct vk_volume_filter f;
    memset(&f, 0, sizeof(f));
    f.op = (int32_t)rnd_below(2u);
    f.flags = rnd_below(2u);
    for (int a = 0; a < 3; a++) {
        f.radius[a] = rnd_below(VK_FILTER_MAX_RADIUS + 1u);
        for (int k = 0; k < 2 * VK_FILTER_MAX_RADIUS + 1; k++) f.weights[a][k] = ((float)rnd_below(2049u) - 1024.0f);
    }
    return f;
}
static void check_validation() {
    struct vk_volume_filter f = random_request();
    const bool have_out = rnd_below(2u) != 0u;
    bool ok = have_out || (f.flags & VK_FILTER_INSTALL);
    CHECK((filter_validate(&f, have_out) == nullptr) == ok, "a valid request");
    CHECK(filter_validate(nullptr, true) != nullptr, "NULL");
    struct vk_volume_filter g = f;
    g.flags |= VK_FILTER_INSTALL;
    switch (rnd_below(7u)) {
        case 0: g.op = 2 + (int32_t)rnd_below(100u); ok = false; break;
        case 1: g.op = -1 - (int32_t)rnd_below(100u); ok = false; break;
        case 2: g.flags |= 2u << rnd_below(31u); ok = false; break;
        case 3: g.radius[rnd_below(3u)] = VK_FILTER_MAX_RADIUS + 1u + rnd_below(1000u); ok = g.op == VK_FILTER_MEDIAN3; break;
        case 4: {  // a used weight beyond the bound or not finite; an unused one is ignored
            const uint32_t a = rnd_below(3u), k = rnd_below(2u * VK_FILTER_MAX_RADIUS + 1u);
            const float bad[5] = {NAN, INFINITY, -INFINITY, 1024.5f, -1025.0f};
            g.weights[a][k] = bad[rnd_below(5u)];
            ok = g.op == VK_FILTER_MEDIAN3 || g.radius[a] == 0u || k > 2u * g.radius[a];
            break;
        }
        case 5: g.weights[rnd_below(3u)][rnd_below(13u)] = rnd_below(2u) ? 1024.0f : -1024.0f; ok = true; break;  // the bound itself is allowed
        default: ok = true; break;
    }
    CHECK((filter_validate(&g, false) == nullptr) == ok, "a modified request (op %d flags %#x)", g.op, g.flags);
}

static void check_gaussian() {
    float w[2 * VK_FILTER_MAX_RADIUS + 1 + 2];
    const uint32_t r = 1u + rnd_below(VK_FILTER_MAX_RADIUS);
    const double sigma = 0.05 + (double)rnd_below(1000u) / 100.0;
    for (float &x : w) x = -7.0f;
    CHECK(filter_gaussian(sigma, r, w + 1) == nullptr, "valid");
    CHECK(w[0] == -7.0f && w[2u * r + 2u] == -7.0f, "writes 2 r + 1 weights");
    double sum = 0.0;
    for (uint32_t k = 0; k <= 2u * r; k++) {
        CHECK(w[1u + k] == w[1u + 2u * r - k] && w[1u + k] >= 0.0f, "symmetric, not negative");
        sum += (double)w[1u + k];
    }
    CHECK(fabs(sum - 1.0) <= (2.0 * r + 1.0) * ldexp(1.0, -24), "sum %a", sum);
    CHECK(filter_gaussian(0.0, r, w) && filter_gaussian(-1.0, r, w) && filter_gaussian(NAN, r, w) && filter_gaussian(INFINITY, r, w), "sigma");
    CHECK(filter_gaussian(1.0, 0u, w) && filter_gaussian(1.0, VK_FILTER_MAX_RADIUS + 1u, w) && filter_gaussian(1.0, r, nullptr), "radius, NULL");
}

int main(int argc, char **argv) {
    if (argc != 3) {
        std::printf("usage: filter_fuzz CASES SEED\n");
        return 2;
    }
    const long cases = std::strtol(argv[1], nullptr, 0);
    g_state = std::strtoull(argv[2], nullptr, 0) | 1ull;
    CHECK(filter_class(0u) == 0u && filter_class(2u) == 0u && filter_class(3u) == 1u && filter_class(4u) == 1u && filter_class(5u) == 2u && filter_class(6u) == 2u, "classes");
    for (uint32_t r = 0; r <= VK_FILTER_MAX_RADIUS; r++) CHECK(kFilterTiles[filter_class(r)].r >= r, "the class of a radius holds it");
    for (uint32_t d = 1; d <= kFilterDivMaxD; d++)  // the divide-free index arithmetic over its whole range
        for (uint32_t n = 0; n < kFilterDivMaxN; n++) CHECK(filter_div(n, filter_div_magic(d)) == n / d, "filter_div(%u, %u)", n, d);
    for (long c = 0; c < cases; c++) {
        const uint32_t nx = random_dim(), ny = random_dim(), nz = random_dim();
        const uint32_t rx = rnd_below(VK_FILTER_MAX_RADIUS + 1u), ry = rnd_below(VK_FILTER_MAX_RADIUS + 1u), rz = rnd_below(VK_FILTER_MAX_RADIUS + 1u);
        const uint32_t cls = filter_class(std::max(rx, std::max(ry, rz)));
        const uint32_t cap = rnd_below(3u) == 0u ? 1u + rnd_below(64u) : 0u;
        check_tiles(nx, ny, nz, kFilterTiles[cls], rx, ry, rz, cap, 4u);
        check_tiles(nx, ny, nz, kMedianTile, 1u, 1u, 1u, cap, 2u);
        check_tiles(8192u, 8192u, 8192u, kFilterTiles[cls], rx, ry, rz, 0u, 4u);
        const uint32_t sx = 1u + rnd_below(70u), sy = 1u + rnd_below(20u), sz = 1u + rnd_below(20u);
        check_cover_brute(sx, sy, sz, kFilterTiles[rnd_below(kFilterClasses)]);
        check_cover_brute(sx, sy, sz, kMedianTile);
        for (int k = 0; k < 200; k++) {
            check_clamp();
            check_store_f16();
            check_store_unorm();
            check_keys();
            check_median();
        }
        for (int k = 0; k < 20; k++) check_validation();
        check_gaussian();
    }
    std::printf("OK (%ld cases)\n", cases);
    return 0;
}
