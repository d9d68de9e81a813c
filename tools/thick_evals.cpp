// thick_evals.cpp -- the work of vk_local_thickness' gather kernel, counted on the host (measurement (c)): the
// kernel's walk replayed tile by tile with vk_thick.hpp's own helpers, in the kernel's order (the output tile first, then the window in
// raster order), over the distance array the library produced.  Built as a shared library by tools/thick_quick.py --count:
//     g++ -O2 -fopenmp -shared -fPIC -I vokselis_amd/csrc -o libthick_evals.so tools/thick_evals.cpp
// counts[0] tile pairs tested, [1] tile pairs accepted, [2] list entries (kept centres) over all accepted pairs, [3] centre evaluations:
// entries times the 512 threads of a workgroup, which all run the list, [4] tiles that walk at all.  Returns the number of voxels whose
// replayed T2 differs from t2 (0: the replay is the kernel's result).
#include "vk_thick.hpp"

#include <algorithm>
#include <vector>

using namespace vk;

static uint64_t voxel_at(uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny) { return (uint64_t)x + (uint64_t)nx * ((uint64_t)y + (uint64_t)ny * z); }

extern "C" uint64_t thick_count(const uint32_t *d2, const uint32_t *t2, uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t *w, uint32_t cap, uint64_t *counts) {
    const uint32_t ntx = thick_tiles_along(nx), nty = thick_tiles_along(ny), ntz = thick_tiles_along(nz), tiles = ntx * nty * ntz;
    uint32_t reach[3];
    for (int c = 0; c < 3; c++) reach[c] = thick_reach(cap, w[c]);
    auto dc_at = [&](uint32_t x, uint32_t y, uint32_t z) { const uint32_t d = d2[voxel_at(x, y, z, nx, ny)]; return d < cap ? d : cap; };
    std::vector<uint32_t> tile_max(tiles, 0u);
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t t = 0; t < (int64_t)tiles; t++) {
        uint32_t tx, ty, tz;
        tile_coords((uint32_t)t, ntx, nty, tx, ty, tz);
        const ThickBox b = thick_tile_box(tx, ty, tz, nx, ny, nz);
        uint32_t top = 0u;
        for (uint32_t z = b.lo[2]; z <= b.hi[2]; z++) for (uint32_t y = b.lo[1]; y <= b.hi[1]; y++) for (uint32_t x = b.lo[0]; x <= b.hi[0]; x++) top = std::max(top, dc_at(x, y, z));
        tile_max[(size_t)t] = top;
    }
    uint64_t tested = 0, accepted = 0, entries = 0, walking = 0, wrong = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : tested, accepted, entries, walking, wrong)
    for (int64_t t = 0; t < (int64_t)tiles; t++) {
        uint32_t tx, ty, tz;
        tile_coords((uint32_t)t, ntx, nty, tx, ty, tz);
        const ThickBox out = thick_tile_box(tx, ty, tz, nx, ny, nz);
        struct Voxel { int32_t q[3]; uint32_t best; bool fg; uint64_t at; };
        std::vector<Voxel> mine;
        for (uint32_t z = out.lo[2]; z <= out.hi[2]; z++) for (uint32_t y = out.lo[1]; y <= out.hi[1]; y++) for (uint32_t x = out.lo[0]; x <= out.hi[0]; x++) {
            const uint32_t dc = dc_at(x, y, z);
            mine.push_back(Voxel{{(int32_t)(w[0] * x), (int32_t)(w[1] * y), (int32_t)(w[2] * z)}, dc, dc != 0u, voxel_at(x, y, z, nx, ny)});
        }
        auto low = [&] {
            uint32_t l = 0xffffffffu;
            for (const Voxel &v : mine)
                if (v.fg) l = std::min(l, v.best);
            return l;
        };
        uint32_t lowest = low();
        if (lowest != 0xffffffffu && lowest < cap) {
            walking++;
            uint32_t f[3], g[3];
            thick_window(tx, ntx, reach[0], f[0], g[0]);
            thick_window(ty, nty, reach[1], f[1], g[1]);
            thick_window(tz, ntz, reach[2], f[2], g[2]);
            const uint32_t wx = g[0] - f[0] + 1u, wy = g[1] - f[1] + 1u, wz = g[2] - f[2] + 1u, steps = wx * wy * wz;
            struct Entry { int32_t p[3]; uint32_t dc; };
            std::vector<Entry> list;
            for (uint32_t j = 0; j <= steps && lowest < cap; j++) {
                uint32_t sx = tx, sy = ty, sz = tz;
                if (j > 0u) {
                    const uint32_t k = j - 1u, row = k / wx;
                    sx = f[0] + (k - row * wx); sz = f[2] + row / wy; sy = f[1] + (row - (row / wy) * wy);
                    if (sx == tx && sy == ty && sz == tz) continue;
                }
                tested++;
                const ThickBox src = thick_tile_box(sx, sy, sz, nx, ny, nz);
                if (thick_tile_skipped(tile_max[thick_tile_index(sx, sy, sz, ntx, nty)], thick_box_box_d2(src, out, w), lowest)) continue;
                accepted++;
                list.clear();
                for (uint32_t z = src.lo[2]; z <= src.hi[2]; z++) for (uint32_t y = src.lo[1]; y <= src.hi[1]; y++) for (uint32_t x = src.lo[0]; x <= src.hi[0]; x++) {
                    const uint32_t dc = dc_at(x, y, z);
                    if (dc && thick_centre_kept(dc, thick_voxel_box_d2(x, y, z, out, w), lowest)) list.push_back(Entry{{(int32_t)(w[0] * x), (int32_t)(w[1] * y), (int32_t)(w[2] * z)}, dc});
                }
                entries += list.size();
                for (Voxel &v : mine)
                    for (const Entry &e : list)
                        if (thick_d2(e.p[0], e.p[1], e.p[2], v.q[0], v.q[1], v.q[2]) < e.dc && e.dc > v.best) v.best = e.dc;
                lowest = low();
            }
        }
        for (const Voxel &v : mine) wrong += t2[v.at] != (v.fg ? v.best : 0u);
    }
    counts[0] = tested; counts[1] = accepted; counts[2] = entries; counts[3] = entries * kThickThreads; counts[4] = walking;
    return wrong;
}
