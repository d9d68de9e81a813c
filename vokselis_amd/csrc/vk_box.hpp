// vk_box.hpp -- a voxel box against a volume, for every pass that works on one (the histogram, the mesh extraction): whether a caller's
// box is valid, its voxel count, the clip box as a voxel box; the index of a voxel in a dense x-fastest array, and a tile's coordinates
// from its number (the thickness, geodesic and skeleton passes, and tests/thick_fuzz.cpp and tools/thick_evals.cpp).  Host and device,
// no HIP in the host part: shared with the host fuzzes (tests/hist_fuzz.cpp, tests/mesh_fuzz.cpp, plain g++ under ASan / UBSan).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/vokselis_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VK_BOX_HD __host__ __device__ __forceinline__
#else
#define VK_BOX_HD inline
#endif

namespace vk {

// voxel (x, y, z) of a dense array of nx x ny x nz, x fastest: the LINEAR layouts, and every dense output
VK_BOX_HD uint64_t voxel_index(uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny) { return (uint64_t)x + (uint64_t)nx * ((uint64_t)y + (uint64_t)ny * (uint64_t)z); }
// ... and back, for a pass that cuts the volume into tiles: tile number t of ntx x nty x ... tiles, x fastest, as its three (the counts by
// reference: a kernel that keeps them in its descriptor reads them where the divisions stand, as if they were written there)
VK_BOX_HD void tile_coords(uint32_t t, const uint32_t &ntx, const uint32_t &nty, uint32_t &tx, uint32_t &ty, uint32_t &tz) {
    const uint32_t row = t / ntx;
    tx = t - row * ntx;
    tz = row / nty;
    ty = row - tz * nty;
}

// A box against the volume: not inverted, inside.
inline bool voxel_box_ok(const vk_voxel_box &b, uint32_t nx, uint32_t ny, uint32_t nz) {
    return b.x0 <= b.x1 && b.y0 <= b.y1 && b.z0 <= b.z1 && b.x1 <= nx && b.y1 <= ny && b.z1 <= nz;
}
inline uint64_t voxel_box_voxels(const vk_voxel_box &b) { return (uint64_t)(b.x1 - b.x0) * (uint64_t)(b.y1 - b.y0) * (uint64_t)(b.z1 - b.z0); }

// One axis of the clip box as an index range [i0, i1): the voxels i of n whose centre (i + 0.5) / n, formed in double, lies in [lo, hi].
// The estimate from lo n - 0.5 is moved until the predicate itself holds on one side and fails on the other (it is monotone in i).
inline bool voxel_centre_ge(uint32_t i, uint32_t n, float lo) { return ((double)i + 0.5) / (double)n >= (double)lo; }
inline bool voxel_centre_le(uint32_t i, uint32_t n, float hi) { return ((double)i + 0.5) / (double)n <= (double)hi; }
inline void voxel_clip_axis(float lo, float hi, uint32_t n, uint32_t &i0, uint32_t &i1) {
    double a = ceil((double)lo * (double)n - 0.5), b = floor((double)hi * (double)n - 0.5) + 1.0;
    a = a < 0.0 ? 0.0 : (a > (double)n ? (double)n : a);
    b = b < 0.0 ? 0.0 : (b > (double)n ? (double)n : b);
    i0 = (uint32_t)a;
    i1 = (uint32_t)b;
    while (i0 > 0u && voxel_centre_ge(i0 - 1u, n, lo)) i0--;
    while (i0 < n && !voxel_centre_ge(i0, n, lo)) i0++;
    while (i1 < n && voxel_centre_le(i1, n, hi)) i1++;
    while (i1 > 0u && !voxel_centre_le(i1 - 1u, n, hi)) i1--;
    if (i1 < i0) i1 = i0;  // no centre inside: an empty range
}
inline vk_voxel_box voxel_clip_box(const float lo[3], const float hi[3], uint32_t nx, uint32_t ny, uint32_t nz) {
    vk_voxel_box b;
    voxel_clip_axis(lo[0], hi[0], nx, b.x0, b.x1);
    voxel_clip_axis(lo[1], hi[1], ny, b.y0, b.y1);
    voxel_clip_axis(lo[2], hi[2], nz, b.z0, b.z1);
    return b;
}

}  // namespace vk
