// vk_label.hpp -- connected components of a value range (vk_label_components): the validation of a caller's
// vk_label_request, the predicate, the neighbour offsets, the union-find over a parent array (find, union), the tile, seam and chunk
// arithmetic, the selection and the fill, shared by the kernels and their host (vk_launch_label.hip) and the host fuzz
// (tests/label_fuzz.cpp, plain g++ under ASan / UBSan, with std::atomic in place of the device atomics).
//
// The parent array.  p[i] of a foreground voxel i is a foreground voxel of the same component with p[i] <= i; p[i] == i makes i a root;
// a background voxel holds kLabelBackground.  Links only ever move to smaller indices, so a root is the smallest index its tree has
// seen and, once every adjacency has been united, the smallest linear index of its component: `first`, and with it the numbering,
// falls out of the structure whatever order the atomics arrive in.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vokselis_hip.h"
#include "vk_box.hpp"
#include "vk_filter.hpp"  // FilterTile, filter_grid, filter_tile_origin; the store rule of the three formats (the fill)

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VK_LABEL_HD __host__ __device__ __forceinline__
#else
#define VK_LABEL_HD inline
#endif

#include <algorithm>
#include <vector>

namespace vk {

constexpr uint32_t kLabelBackground = 0xffffffffu;     // p[i] of a voxel that is not foreground
constexpr uint64_t kLabelMaxVoxels = 0xfffffffeull;    // indices and ids are 32-bit: 0 is "no component", 0xffffffff "background"

// ---- the request -------------------------------------------------------------------------------------------------------------
// A caller's request without the volume (seeds and box are checked against it by the entry point).  Returns nullptr, or what is wrong
// (VK_ERR_INVALID).
inline const char *label_validate(const vk_label_request *r, bool have_labels, bool have_components, uint64_t cap_components, bool have_dense, bool have_result) {
    if (!r) return "the request is NULL";
    if (isnan(r->lo) || isnan(r->hi)) return "lo or hi is NaN";
    if (r->lo > r->hi) return "lo > hi";
    if (!isfinite(r->fill)) return "fill is not finite";
    if (r->connectivity != 6u && r->connectivity != 18u && r->connectivity != 26u) return "connectivity must be 6, 18 or 26";
    if (r->flags & ~(uint32_t)(VK_LABEL_CLIP_BOX | VK_LABEL_INSTALL | VK_LABEL_INVERT)) return "unknown flag (VK_LABEL_CLIP_BOX, VK_LABEL_INSTALL, VK_LABEL_INVERT)";
    if (r->keep < VK_LABEL_KEEP_ALL || r->keep > VK_LABEL_KEEP_SEEDS) return "unknown keep value (VK_LABEL_KEEP_ALL, _LARGEST, _MIN_SIZE, _SEEDS)";
    if (r->pad != 0u) return "pad must be 0";
    const bool counted = r->keep == VK_LABEL_KEEP_LARGEST || r->keep == VK_LABEL_KEEP_MIN_SIZE;
    if (counted ? r->count < 1u : r->count != 0u) return "count does not fit the keep mode (KEEP_LARGEST, KEEP_MIN_SIZE: >= 1; otherwise 0)";
    if (r->keep == VK_LABEL_KEEP_SEEDS ? (r->n_seeds < 1u || r->n_seeds > (uint32_t)VK_LABEL_MAX_SEEDS) : r->n_seeds != 0u)
        return "n_seeds does not fit the keep mode (KEEP_SEEDS: 1 .. VK_LABEL_MAX_SEEDS; otherwise 0)";
    if (have_components && cap_components == 0u) return "components with cap_components == 0";
    if (!have_labels && !have_components && !have_dense && !have_result && !(r->flags & VK_LABEL_INSTALL))
        return "none of labels_out, components, dense_out, VK_LABEL_INSTALL and result: the result would go nowhere";
    return nullptr;
}
// Whether a volume's voxels can be indexed and numbered in 32 bits: at most kLabelMaxVoxels = 2^32 - 2 (VK_ERR_UNSUPPORTED otherwise).
inline bool label_volume_fits(uint32_t nx, uint32_t ny, uint32_t nz) { return (uint64_t)nx * ny * nz <= kLabelMaxVoxels; }
inline bool label_seeds_inside(const vk_label_request *r, uint32_t nx, uint32_t ny, uint32_t nz) {
    for (uint32_t s = 0; s < r->n_seeds; s++)
        if (r->seeds[s][0] >= nx || r->seeds[s][1] >= ny || r->seeds[s][2] >= nz) return false;
    return true;
}

// lo and hi on the kernel's scale, as vk_set_isosurface forms iso_k; format: VK_FMT_*
inline float label_scale_bound(float v, int format) { return format == VK_FMT_R8_UNORM ? v * 255.0f : (format == VK_FMT_R16_UNORM ? v * 65535.0f : v); }
// F: the fill through the filter's store rule
inline uint32_t label_fill_bits(float fill, int format) {
    return format == VK_FMT_R8_UNORM ? filter_store_unorm(fill * 255.0f, 255.0f) : (format == VK_FMT_R16_UNORM ? filter_store_unorm(fill * 65535.0f, 65535.0f) : filter_store_f16(fill));
}
// the predicate: false for a NaN
VK_LABEL_HD bool label_foreground(float t, float lo_k, float hi_k) { return t >= lo_k && t <= hi_k; }

// ---- neighbours --------------------------------------------------------------------------------------------------------------
// Offset k = 0 .. 26 of the 3x3x3 neighbourhood: d = (k % 3 - 1, k / 3 % 3 - 1, k / 9 - 1); 13 is the voxel itself, and the offsets
// below 13 are the neighbours that come earlier in raster order.  conn_sum: 1, 2, 3 for connectivity 6, 18, 26.
constexpr uint32_t kLabelOffsets = 27, kLabelCentre = 13;
VK_LABEL_HD uint32_t label_conn_sum(uint32_t connectivity) { return connectivity == 6u ? 1u : (connectivity == 18u ? 2u : 3u); }
VK_LABEL_HD void label_offset(uint32_t k, int &dx, int &dy, int &dz) {
    dx = (int)(k % 3u) - 1;
    dy = (int)(k / 3u % 3u) - 1;
    dz = (int)(k / 9u) - 1;
}
VK_LABEL_HD bool label_adjacent(int dx, int dy, int dz, uint32_t conn_sum) {
    const uint32_t s = (uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz));
    return s >= 1u && s <= conn_sum;
}

// ---- the union-find ----------------------------------------------------------------------------------------------------------
// A: how the parent array is read and lowered -- A::load(p, i) and A::fetch_min(p, i, v), which returns the value before.  The device
// has one for LDS and one for global memory (vk_launch_label.hip), the host fuzz one on std::atomic.
//
// Neither function waits for anybody: every trip of either loop makes progress of its own.  A load may return an OLDER value of
// p[i] than the newest (another XCD's L2, a CU's L1): every value p[i] ever held is a voxel of i's component with value <= i, so a
// stale load names an ancestor further up the same tree, costs trips and never correctness -- what decides a union is the value
// fetch_min returns.
template <class A, class P>
VK_LABEL_HD uint32_t label_find(P p, uint32_t i) {
    // decreases strictly: i, as q < i on every trip that goes on.  At most i + 1 loads.
    for (;;) {
        const uint32_t q = A::load(p, i);
        if (q >= i) return i;  // a root (q == i)
        i = q;
    }
}
// Unites the components of the foreground voxels a and b.
template <class A, class P>
VK_LABEL_HD void label_union(P p, uint32_t a, uint32_t b) {
    // decreases strictly: a + b.  The finds never raise a or b, and a trip that goes on replaces the larger of the two, a, by old < a --
    // fetch_min found p[a] != a, which only happens after another union has lowered it.  At most a + b + 1 trips.
    for (;;) {
        a = label_find<A>(p, a);
        b = label_find<A>(p, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = A::fetch_min(p, a, b);
        if (old >= a) return;  // old == a: a was a root and now hangs under b (old > a does not occur: p[a] <= a)
        // a had a parent `old` already.  p[a] is now min(old, b), a voxel of the united component either way; what is left to unite is old with b.
        a = old;
    }
}

// ---- tiles -------------------------------------------------------------------------------------------------------------------
// A 256-thread workgroup owns a tile of 32 x 16 x 8 voxels, 16 per thread, and resolves it in LDS: a row of 32 along x keeps the loads
// of a half wave in one line, 4096 labels are 16 KiB of LDS, and 22 % of a tile's voxels lie on its three low faces -- the seam kernel's
// work -- against 28 % of a 32 x 8 x 8 tile.  The local index of a voxel is x fastest like the volume's, so the order of two voxels of
// one tile is the order of their linear indices and the smallest local index of a set is its smallest global one.
constexpr uint32_t kLabelThreads = 256;
constexpr FilterTile kLabelTile = {32u, 16u, 8u, 0u};
constexpr uint32_t kLabelTileVoxels = kLabelTile.tx * kLabelTile.ty * kLabelTile.tz;
constexpr uint32_t kLabelPerThread = kLabelTileVoxels / kLabelThreads;
static_assert(kLabelTileVoxels % kLabelThreads == 0, "a tile's voxels are a multiple of the workgroup");
VK_LABEL_HD uint32_t label_local_index(uint32_t lx, uint32_t ly, uint32_t lz) { return lx + kLabelTile.tx * (ly + kLabelTile.ty * lz); }
VK_LABEL_HD void label_local_coords(uint32_t e, uint32_t &lx, uint32_t &ly, uint32_t &lz) {
    lx = e % kLabelTile.tx;
    ly = e / kLabelTile.tx % kLabelTile.ty;
    lz = e / (kLabelTile.tx * kLabelTile.ty);
}
VK_LABEL_HD bool label_in_tile(int lx, int ly, int lz) {
    return lx >= 0 && ly >= 0 && lz >= 0 && lx < (int)kLabelTile.tx && ly < (int)kLabelTile.ty && lz < (int)kLabelTile.tz;
}
VK_LABEL_HD bool label_in_box(uint32_t x, uint32_t y, uint32_t z, const vk_voxel_box &b) { return x >= b.x0 && x < b.x1 && y >= b.y0 && y < b.y1 && z >= b.z0 && z < b.z1; }

// ---- seams -------------------------------------------------------------------------------------------------------------------
// The adjacencies between two tiles.  The pair (v, v + d) is the work of the end whose tile comes LATER in the order of tiles: of v iff
// on the highest axis (z, then y, then x) on which the two tiles differ v + d lies below.  Such a v sits on a low face of its tile, so the
// seam kernel visits the voxels of the three low faces, each once:
//     e <  tx ty                       (e % tx, e / tx, 0)                         the face z = 0
//     e' = e - tx ty < tx (tz - 1)     (e' % tx, 0, 1 + e' / tx)                   the face y = 0 without its row on z = 0
//     e'' = e' - tx (tz - 1)           (0, 1 + e'' % (ty - 1), 1 + e'' / (ty - 1)) the face x = 0 without what the other two hold
constexpr uint32_t kLabelSeamVoxels = kLabelTile.tx * kLabelTile.ty + kLabelTile.tx * (kLabelTile.tz - 1u) + (kLabelTile.ty - 1u) * (kLabelTile.tz - 1u);
VK_LABEL_HD void label_seam_voxel(uint32_t e, uint32_t &lx, uint32_t &ly, uint32_t &lz) {
    if (e < kLabelTile.tx * kLabelTile.ty) { lx = e % kLabelTile.tx; ly = e / kLabelTile.tx; lz = 0u; return; }
    e -= kLabelTile.tx * kLabelTile.ty;
    if (e < kLabelTile.tx * (kLabelTile.tz - 1u)) { lx = e % kLabelTile.tx; ly = 0u; lz = 1u + e / kLabelTile.tx; return; }
    e -= kLabelTile.tx * (kLabelTile.tz - 1u);
    lx = 0u; ly = 1u + e % (kLabelTile.ty - 1u); lz = 1u + e / (kLabelTile.ty - 1u);
}
VK_LABEL_HD int label_tile_step(int l, uint32_t extent) { return l < 0 ? -1 : (l >= (int)extent ? 1 : 0); }
VK_LABEL_HD bool label_seam_owner(uint32_t lx, uint32_t ly, uint32_t lz, int dx, int dy, int dz) {
    const int cx = label_tile_step((int)lx + dx, kLabelTile.tx), cy = label_tile_step((int)ly + dy, kLabelTile.ty), cz = label_tile_step((int)lz + dz, kLabelTile.tz);
    return cz ? cz < 0 : (cy ? cy < 0 : cx < 0);
}

// ---- chunks: flatten, renumber, label ----------------------------------------------------------------------------------------
// The passes over the parent array work in chunks of 4096 consecutive voxels, one chunk per trip of a workgroup.  Roots are counted per
// chunk, the counts are scanned in chunk order, and a root's id is 1 + the roots of earlier chunks + the roots before it in its own:
// an exclusive scan in index order.  In the renumbering a thread takes 16 CONSECUTIVE voxels of the chunk, so that thread order is
// index order.
constexpr uint32_t kLabelChunk = 4096, kLabelChunkPerThread = kLabelChunk / kLabelThreads;
constexpr uint32_t kLabelMaxBlocks = 1u << 22;  // grid-stride kernels: a launch may not exceed 2^32 threads
VK_LABEL_HD uint32_t label_chunks(uint64_t n) { return (uint32_t)((n + kLabelChunk - 1u) / kLabelChunk); }
VK_LABEL_HD uint32_t label_blocks(uint64_t work, uint32_t max_blocks) {
    uint64_t b = work > kLabelMaxBlocks ? kLabelMaxBlocks : work;
    if (max_blocks && b > max_blocks) b = max_blocks;
    return b < 1u ? 1u : (uint32_t)b;
}
// voxel i of a volume nx x ny as coordinates
VK_LABEL_HD void label_coords(uint32_t i, uint32_t nx, uint32_t ny, uint32_t &x, uint32_t &y, uint32_t &z) {
    const uint32_t row = i / nx;
    x = i - row * nx;
    z = row / ny;
    y = row - z * ny;
}

// ---- the selection (host) ----------------------------------------------------------------------------------------------------
// keep[id] for id = 0 .. n (keep[0] = 0: background is never selected) from the sizes of components 1 .. n (sizes[id - 1]) and, under
// KEEP_SEEDS, the labels under the seeds.  Returns the number of selected components; their voxels in *kept_voxels.
inline uint64_t label_select(const vk_label_request &r, const uint32_t *sizes, uint64_t n, const uint32_t *seed_labels, std::vector<uint8_t> &keep, uint64_t *kept_voxels) {
    keep.assign((size_t)n + 1u, 0u);
    if (r.keep == VK_LABEL_KEEP_ALL) {
        for (uint64_t id = 1; id <= n; id++) keep[id] = 1u;
    } else if (r.keep == VK_LABEL_KEEP_MIN_SIZE) {
        for (uint64_t id = 1; id <= n; id++) keep[id] = (uint64_t)sizes[id - 1u] >= r.count;
    } else if (r.keep == VK_LABEL_KEEP_SEEDS) {
        for (uint32_t s = 0; s < r.n_seeds; s++)
            if (seed_labels[s] != 0u && seed_labels[s] <= n) keep[seed_labels[s]] = 1u;
    } else if (r.count >= n) {
        for (uint64_t id = 1; id <= n; id++) keep[id] = 1u;
    } else {  // the first `count` by size descending, then first ascending: ids are in the order of first
        std::vector<uint32_t> order((size_t)n);
        for (uint64_t k = 0; k < n; k++) order[k] = (uint32_t)k;
        auto before = [&](uint32_t a, uint32_t b) { return sizes[a] != sizes[b] ? sizes[a] > sizes[b] : a < b; };
        std::partial_sort(order.begin(), order.begin() + (ptrdiff_t)r.count, order.end(), before);
        for (uint64_t k = 0; k < r.count; k++) keep[(size_t)order[k] + 1u] = 1u;
    }
    uint64_t comps = 0, voxels = 0;
    for (uint64_t id = 1; id <= n; id++)
        if (keep[id]) { comps++; voxels += sizes[id - 1u]; }
    *kept_voxels = voxels;
    return comps;
}

}  // namespace vk
