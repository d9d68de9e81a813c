// vk_thick.hpp -- local thickness of a value range (vk_local_thickness): the validation of a caller's
// vk_thickness_request in its order, the cap C, the reach of a ball along an axis, the squared distances between two boxes and between
// a voxel and a box over a spacing, and the tile arithmetic of the gather, for the kernels and their host (vk_launch_thick.hip); plain
// C++ that g++ compiles without a device, so that the host fuzz (tests/thick_fuzz.cpp) shares it.  The predicate and the fill are the
// label pass's (vk_label.hpp); the overflow bound is the distance pass's (vk_dist.hpp).
//
// The gather.  The volume is cut into tiles of 8^3 voxels.  A workgroup owns an output tile and keeps one running T2 per voxel, which
// starts at Dc(v).  A centre u raises a voxel v when d2(u, v) < Dc(u), so a source tile whose largest Dc is not above the squared
// distance between the two tiles' boxes holds no centre that reaches the output tile (thick_tile_skipped), and a centre whose Dc is not
// above its squared distance to the output tile's box reaches none of its voxels (thick_centre_kept).  Both distances are lower bounds
// of d2(u, v) over the voxels they stand for: a skip never drops a ball that reaches.  A source tile or centre whose Dc is not above
// the smallest running T2 of the output tile's foreground voxels can raise nothing either: max commutes, so the order of the walk is free.
#pragma once

#include "vk_box.hpp"
#include "vk_dist.hpp"

namespace vk {

constexpr uint32_t kThickTile = 8, kThickTileVoxels = kThickTile * kThickTile * kThickTile;
constexpr uint32_t kThickThreads = kThickTileVoxels;  // a voxel per thread
constexpr uint64_t kThickMaxC = (uint64_t)(VK_THICK_MAX_REACH * VK_DIST_MAX_SPACING) * (uint64_t)(VK_THICK_MAX_REACH * VK_DIST_MAX_SPACING);  // 2^22
// the source tiles along an axis that a ball of the largest reach can lie in: the output tile, and (32 + 7) / 8 tiles on each side
constexpr uint32_t kThickMaxWindow = 2u * ((VK_THICK_MAX_REACH + kThickTile - 1u) / kThickTile) + 1u;
static_assert(kThickMaxWindow <= 2u * VK_THICK_MAX_REACH / kThickTile + 3u, "the window stays within (2 * 32 / 8 + 3) tiles per axis");

// ---- the request -------------------------------------------------------------------------------------------------------------
inline uint32_t thick_min_spacing(const uint32_t spacing[3]) {
    const uint32_t m = spacing[0] < spacing[1] ? spacing[0] : spacing[1];
    return m < spacing[2] ? m : spacing[2];
}
// A caller's request without the volume (the box, the volume's kind and the overflow bound are the entry point's).  Returns nullptr,
// or what is wrong (VK_ERR_INVALID): the first of the header's list that applies.
inline const char *thick_validate(const vk_thickness_request *r, bool have_t2, bool have_dense, bool have_result) {
    if (!r) return "the request is NULL";
    if (isnan(r->lo) || isnan(r->hi)) return "lo or hi is NaN";
    if (r->lo > r->hi) return "lo > hi";
    if (r->flags & ~(uint32_t)(VK_THICK_CLIP_BOX | VK_THICK_INSTALL)) return "unknown flag (VK_THICK_CLIP_BOX, VK_THICK_INSTALL)";
    for (int c = 0; c < 3; c++)
        if (r->spacing[c] < 1u || r->spacing[c] > (uint32_t)VK_DIST_MAX_SPACING) return "a spacing outside 1 .. VK_DIST_MAX_SPACING";
    if (!isfinite(r->max_radius) || r->max_radius < 1.0f) return "max_radius is not finite or lies below 1";
    if (r->max_radius / (float)thick_min_spacing(r->spacing) > (float)VK_THICK_MAX_REACH) return "max_radius reaches further than VK_THICK_MAX_REACH voxels of the smallest spacing";
    if (!isfinite(r->gain) || r->gain < 0.0f) return "gain is negative or not finite";
    if (!isfinite(r->fill_out)) return "fill_out is not finite";
    if (!have_t2 && !have_dense && !have_result && !(r->flags & VK_THICK_INSTALL)) return "none of t2_out, dense_out, VK_THICK_INSTALL and result: the result would go nowhere";
    return nullptr;
}
// C: 1 <= C <= kThickMaxC for a request that passed
inline uint64_t thick_cap(float max_radius) { return (uint64_t)floor((double)max_radius * (double)max_radius); }
// the largest k with (w k)^2 < C: how many voxels along an axis of pitch w the centre of a ball that holds a voxel can lie away.
// At most VK_THICK_MAX_REACH for a request that passed: sqrt(C) <= max_radius <= 32 min_c w.
inline uint32_t thick_reach(uint64_t C, uint32_t w) {
    uint32_t k = 0u;
    while (k < (uint32_t)VK_THICK_MAX_REACH * (uint32_t)VK_DIST_MAX_SPACING && (uint64_t)w * (k + 1u) * ((uint64_t)w * (k + 1u)) < C) k++;
    return k;
}
// the automatic gain
inline float thick_auto_gain(uint32_t max_t2) { return max_t2 ? 1.0f / sqrtf((float)max_t2) : 0.0f; }

// ---- boxes and distances -------------------------------------------------------------------------------------------------------
// A box of voxels, inclusive on both ends, inside the volume.
struct ThickBox { uint32_t lo[3], hi[3]; };
// tile t (tx, ty, tz) of a volume of n voxels per axis, clipped to it
VK_DIST_HD ThickBox thick_tile_box(uint32_t tx, uint32_t ty, uint32_t tz, uint32_t nx, uint32_t ny, uint32_t nz) {
    ThickBox b;
    const uint32_t t[3] = {tx, ty, tz}, n[3] = {nx, ny, nz};
    for (int c = 0; c < 3; c++) {
        b.lo[c] = t[c] * kThickTile;
        const uint32_t end = b.lo[c] + kThickTile - 1u;
        b.hi[c] = end < n[c] - 1u ? end : n[c] - 1u;
    }
    return b;
}
// the steps between the intervals [a0, a1] and [b0, b1]: 0 where they overlap
VK_DIST_HD uint32_t thick_gap(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) { return b0 > a1 ? b0 - a1 : (a0 > b1 ? a0 - b1 : 0u); }
// min over u in a, v in b of d2(u, v)
VK_DIST_HD uint64_t thick_box_box_d2(const ThickBox &a, const ThickBox &b, const uint32_t w[3]) {
    uint64_t s = 0;
    for (int c = 0; c < 3; c++) {
        const uint64_t g = (uint64_t)w[c] * thick_gap(a.lo[c], a.hi[c], b.lo[c], b.hi[c]);
        s += g * g;
    }
    return s;
}
// min over v in b of d2(u, v)
VK_DIST_HD uint64_t thick_voxel_box_d2(uint32_t ux, uint32_t uy, uint32_t uz, const ThickBox &b, const uint32_t w[3]) {
    const uint32_t u[3] = {ux, uy, uz};
    uint64_t s = 0;
    for (int c = 0; c < 3; c++) {
        const uint64_t g = (uint64_t)w[c] * thick_gap(u[c], u[c], b.lo[c], b.hi[c]);
        s += g * g;
    }
    return s;
}
// d2(u, v) from the positions w_c u_c and w_c v_c, each below 2^16 under dist_d2_fits, as is the sum's fit in 32 bits
VK_DIST_HD uint32_t thick_d2(int32_t px, int32_t py, int32_t pz, int32_t qx, int32_t qy, int32_t qz) {
    const int32_t dx = px - qx, dy = py - qy, dz = pz - qz;
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__mul24(dx, dx) + (uint32_t)__mul24(dy, dy) + (uint32_t)__mul24(dz, dz);  // |d| < 2^16: 24-bit factors, the low 32 bits of the product
#else
    return (uint32_t)((int64_t)dx * dx) + (uint32_t)((int64_t)dy * dy) + (uint32_t)((int64_t)dz * dz);
#endif
}

// ---- the two skips and the window ------------------------------------------------------------------------------------------------
// No centre of a source tile whose largest Dc is tile_max reaches the output tile, or can raise a running T2 that is >= lowest everywhere.
VK_DIST_HD bool thick_tile_skipped(uint32_t tile_max, uint64_t box_d2, uint32_t lowest) { return (uint64_t)tile_max <= box_d2 || tile_max <= lowest; }
// ... and a centre, against its own distance to the output tile's box
VK_DIST_HD bool thick_centre_kept(uint32_t dc, uint64_t voxel_box_d2, uint32_t lowest) { return (uint64_t)dc > voxel_box_d2 && dc > lowest; }
// The source tiles along an axis for output tile t of nt: [first, last], at most kThickMaxWindow of them.  reach: thick_reach.
VK_DIST_HD void thick_window(uint32_t t, uint32_t nt, uint32_t reach, uint32_t &first, uint32_t &last) {
    const uint32_t back = (reach + kThickTile - 1u) / kThickTile;
    first = t > back ? t - back : 0u;
    const uint32_t end = (t * kThickTile + kThickTile - 1u + reach) / kThickTile;
    last = end < nt - 1u ? end : nt - 1u;
}
// a tile's number from its three, x fastest (back: vk_box.hpp, tile_coords)
VK_DIST_HD uint32_t thick_tile_index(uint32_t tx, uint32_t ty, uint32_t tz, uint32_t ntx, uint32_t nty) { return tx + ntx * (ty + nty * tz); }
inline uint32_t thick_tiles_along(uint32_t n) { return (n + kThickTile - 1u) / kThickTile; }

}  // namespace vk
