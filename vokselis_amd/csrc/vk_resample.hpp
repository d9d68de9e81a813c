// vk_resample.hpp -- the resample pass (vk_volume_resample): the validation of a caller's vk_resample_request, the
// integer geometry of the three rules (the NEAREST index, the LINEAR taps and fraction, the AREA tap range and weights), the per-axis
// tables built from it once per call, the value map's constants, the store rule and the grid arithmetic, shared by the kernels and their
// host (vk_launch_resample.hip) and the host fuzz (tests/resample_fuzz.cpp, plain g++ under ASan / UBSan).  No HIP in the host part.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vokselis_hip.h"
#include "vk_box.hpp"
#include "vk_filter.hpp"

#if defined(__HIPCC__)
#define VK_RESAMPLE_HD __host__ __device__ __forceinline__
#else
#define VK_RESAMPLE_HD inline
#endif

namespace vk {

constexpr uint32_t kResampleMaxExtent = 65535u;
constexpr uint32_t kResampleMaxTaps = VK_RESAMPLE_MAX_RATIO + 1u;  // AREA: source voxels an output voxel overlaps per axis, at most

// ---- the geometry of an axis: nb box voxels into n output voxels, 1 <= nb, n <= 65535, j < n -----------------------------------------
// every product below stays under 2^34
VK_RESAMPLE_HD uint32_t resample_nearest(uint32_t j, uint32_t nb, uint32_t n) { return (uint32_t)(((2u * (uint64_t)j + 1u) * nb) / (2u * (uint64_t)n)); }

struct ResampleLinearTap {
    uint32_t i0, i1;  // c(i), c(i + 1)
    float f;
};
VK_RESAMPLE_HD ResampleLinearTap resample_linear(uint32_t j, uint32_t nb, uint32_t n) {
    const int64_t num = (2 * (int64_t)j + 1) * (int64_t)nb - (int64_t)n, den = 2 * (int64_t)n;
    int64_t i = num / den;
    if (num < 0 && i * den != num) i--;  // floor
    const int64_t r = num - i * den;     // 0 <= r < den
    ResampleLinearTap t;
    t.i0 = filter_clamp(i, nb);
    t.i1 = filter_clamp(i + 1, nb);
    t.f = (float)((double)r / (double)den);
    return t;
}

VK_RESAMPLE_HD uint32_t resample_area_first(uint32_t j, uint32_t nb, uint32_t n) { return (uint32_t)(((uint64_t)j * nb) / n); }
VK_RESAMPLE_HD uint32_t resample_area_last(uint32_t j, uint32_t nb, uint32_t n) { return (uint32_t)((((uint64_t)j + 1u) * nb - 1u) / n); }
// the overlap of source voxel k with output voxel j, in units of 1 / n of a box voxel
VK_RESAMPLE_HD uint64_t resample_area_overlap(uint32_t j, uint32_t k, uint32_t nb, uint32_t n) {
    const uint64_t a0 = (uint64_t)j * nb, a1 = ((uint64_t)j + 1u) * nb, b0 = (uint64_t)k * n, b1 = ((uint64_t)k + 1u) * n;
    const uint64_t hi = a1 < b1 ? a1 : b1, lo = a0 > b0 ? a0 : b0;
    return hi > lo ? hi - lo : 0u;
}
VK_RESAMPLE_HD float resample_area_weight(uint32_t j, uint32_t k, uint32_t nb, uint32_t n) { return (float)((double)resample_area_overlap(j, k, nb, n) / (double)nb); }
inline bool resample_area_ratio_ok(uint32_t nb, uint32_t n) { return (uint64_t)nb <= (uint64_t)VK_RESAMPLE_MAX_RATIO * n; }
// the most taps an output voxel of the axis has
inline uint32_t resample_area_max_taps(uint32_t nb, uint32_t n) {
    uint32_t m = 1u;
    for (uint32_t j = 0; j < n; j++) {
        const uint32_t c = resample_area_last(j, nb, n) - resample_area_first(j, nb, n) + 1u;
        m = c > m ? c : m;
    }
    return m;
}

// r where every axis shrinks by the same integer r in 2 .. 4 (nb = r n: every output voxel has exactly r taps per axis, each of weight
// 1 / r); otherwise 0
inline uint32_t resample_uniform_taps(const uint32_t nb[3], const uint32_t n[3]) {
    const uint32_t r = nb[0] / n[0];
    if (r < 2u || r > 4u) return 0u;
    for (int a = 0; a < 3; a++)
        if ((uint64_t)n[a] * r != nb[a]) return 0u;
    return r;
}

// ---- the per-axis tables: one array of 32-bit words per call, the three axes one behind the other -----------------------------------
// NEAREST: n words, the index.  LINEAR: 3 n words, (i0, i1, bits of f) per output voxel.  AREA: 2 n words (first, count), then
// n * taps words, the weights' bits, `taps` (the axis's resample_area_max_taps) per output voxel.
struct ResampleAxis {
    uint32_t nb, n;    // box extent, output extent
    uint32_t base;     // the axis's first word
    uint32_t taps;     // AREA: the weights' stride
};
inline uint64_t resample_axis_words(int mode, uint32_t n, uint32_t taps) {
    return mode == VK_RESAMPLE_NEAREST ? (uint64_t)n : (mode == VK_RESAMPLE_LINEAR ? 3u * (uint64_t)n : (2u + (uint64_t)taps) * n);
}
// lays the three axes out; returns the words of the whole table (at most 3 * 19 * 65535: fits 32 bits)
inline uint32_t resample_table_layout(int mode, const uint32_t nb[3], const uint32_t n[3], ResampleAxis ax[3]) {
    uint64_t at = 0;
    for (int a = 0; a < 3; a++) {
        ax[a].nb = nb[a];
        ax[a].n = n[a];
        ax[a].base = (uint32_t)at;
        ax[a].taps = mode == VK_RESAMPLE_AREA ? resample_area_max_taps(nb[a], n[a]) : 0u;
        at += resample_axis_words(mode, n[a], ax[a].taps);
    }
    return (uint32_t)at;
}
// fills one axis of a table of `words` words
inline void resample_table_fill(int mode, const ResampleAxis &A, uint32_t *table) {
    uint32_t *t = table + A.base;
    for (uint32_t j = 0; j < A.n; j++) {
        if (mode == VK_RESAMPLE_NEAREST) t[j] = resample_nearest(j, A.nb, A.n);
        else if (mode == VK_RESAMPLE_LINEAR) {
            const ResampleLinearTap L = resample_linear(j, A.nb, A.n);
            t[3u * j] = L.i0;
            t[3u * j + 1u] = L.i1;
            t[3u * j + 2u] = filter_f32_bits(L.f);
        } else {
            const uint32_t k0 = resample_area_first(j, A.nb, A.n), k1 = resample_area_last(j, A.nb, A.n);
            t[2u * j] = k0;
            t[2u * j + 1u] = k1 - k0 + 1u;
            uint32_t *w = t + 2u * (size_t)A.n + (size_t)j * A.taps;
            for (uint32_t k = k0; k <= k1; k++) w[k - k0] = filter_f32_bits(resample_area_weight(j, k, A.nb, A.n));
            for (uint32_t k = k1 - k0 + 1u; k < A.taps; k++) w[k] = 0u;
        }
    }
}

// ---- the value map ------------------------------------------------------------------------------------------------------------------
inline double resample_format_scale(int format) { return format == VK_FMT_R8_UNORM ? 255.0 : (format == VK_FMT_R16_UNORM ? 65535.0 : 1.0); }
inline void resample_value_map(int fmt_in, int fmt_out, float lo, float hi, float &a, float &b) {
    const double d = (double)hi - (double)lo, s_in = resample_format_scale(fmt_in), s_out = resample_format_scale(fmt_out);
    a = (float)(s_out / (d * s_in));
    b = (float)(-(double)lo * s_out / d);
}

// ---- the store rule -----------------------------------------------------------------------------------------------------------------
// vk_volume_filter's, with the NaN a resample may meet (an R16F source into an integer format) stored as 0
VK_RESAMPLE_HD uint32_t resample_store_unorm(float v, float top) { return v == v ? filter_store_unorm(v, top) : 0u; }
VK_RESAMPLE_HD float resample_lerp(float a, float b, float f) { return f == 0.0f ? a : fmaf(f, b - a, a); }

// ---- the request --------------------------------------------------------------------------------------------------------------------
inline bool resample_scalar_format(int f) { return f == VK_FMT_R8_UNORM || f == VK_FMT_R16_UNORM || f == VK_FMT_R16_FLOAT; }
// What does not depend on the volume.  Returns nullptr, or what is wrong (VK_ERR_INVALID).  have_out: dense_out is not NULL.
inline const char *resample_validate(const vk_resample_request *r, bool have_out) {
    if (!r) return "the request is NULL";
    if (r->mode != VK_RESAMPLE_NEAREST && r->mode != VK_RESAMPLE_LINEAR && r->mode != VK_RESAMPLE_AREA) return "unknown mode (VK_RESAMPLE_NEAREST, _LINEAR, _AREA)";
    if (r->flags & ~(uint32_t)(VK_RESAMPLE_INSTALL | VK_RESAMPLE_CLIP_BOX | VK_RESAMPLE_WINDOW)) return "unknown flag (VK_RESAMPLE_INSTALL, _CLIP_BOX, _WINDOW)";
    if (r->format == VK_FMT_RGBA16F_PAIR) return "RGBA16F_PAIR is no output format (R8_UNORM, R16_UNORM, R16_FLOAT or VK_RESAMPLE_KEEP_FORMAT)";
    if (r->format != VK_RESAMPLE_KEEP_FORMAT && !resample_scalar_format(r->format)) return "unknown format (R8_UNORM, R16_UNORM, R16_FLOAT or VK_RESAMPLE_KEEP_FORMAT)";
    for (int a = 0; a < 3; a++)
        if (r->dims[a] > kResampleMaxExtent) return "an output extent is above 65535";
    if (r->flags & VK_RESAMPLE_WINDOW) {
        if (!isfinite(r->lo) || !isfinite(r->hi)) return "the window's lo or hi is not finite";
        if (!(r->lo < r->hi)) return "the window needs lo < hi";
    }
    if (!have_out && !(r->flags & VK_RESAMPLE_INSTALL)) return "neither dense_out nor VK_RESAMPLE_INSTALL: the result would go nowhere";
    if ((r->flags & VK_RESAMPLE_INSTALL) && (r->layout < VK_LAYOUT_AUTO || r->layout > VK_LAYOUT_STAGED)) return "unknown layout";
    return nullptr;
}

// What depends on the volume and the box: the output's extents, format and layout, the map.  status: VK_ERR_INVALID or VK_ERR_UNSUPPORTED.
struct ResamplePlan {
    uint32_t nb[3], n[3];
    int format, layout;  // of the output; layout 0 without INSTALL
    bool map;
    float a, b;
};
inline const char *resample_plan(const vk_resample_request *r, const vk_voxel_box &B, int vol_format, int vol_layout, ResamplePlan &P, int &status) {
    status = VK_ERR_INVALID;
    P.nb[0] = B.x1 - B.x0; P.nb[1] = B.y1 - B.y0; P.nb[2] = B.z1 - B.z0;
    for (int a = 0; a < 3; a++) {
        if (P.nb[a] == 0u) return "the box is empty";
        P.n[a] = r->dims[a] ? r->dims[a] : P.nb[a];
        if (P.n[a] > kResampleMaxExtent || P.nb[a] > kResampleMaxExtent) return "an output extent is above 65535";
    }
    P.format = r->format == VK_RESAMPLE_KEEP_FORMAT ? vol_format : r->format;
    const bool window = (r->flags & VK_RESAMPLE_WINDOW) != 0u;
    P.map = P.format != vol_format || window;
    P.a = 1.0f;
    P.b = 0.0f;
    if (P.map) {
        resample_value_map(vol_format, P.format, window ? r->lo : 0.0f, window ? r->hi : 1.0f, P.a, P.b);
        if (!isfinite(P.a) || !isfinite(P.b)) return "the window's a or b is not finite in f32";
    }
    status = VK_ERR_UNSUPPORTED;
    if (r->mode == VK_RESAMPLE_AREA)
        for (int a = 0; a < 3; a++)
            if (!resample_area_ratio_ok(P.nb[a], P.n[a])) return "VK_RESAMPLE_AREA shrinks an axis by more than VK_RESAMPLE_MAX_RATIO (resample in two steps)";
    P.layout = 0;
    if (r->flags & VK_RESAMPLE_INSTALL) {
        P.layout = r->layout;
        if (P.layout == VK_LAYOUT_AUTO) P.layout = (vol_layout == VK_LAYOUT_PACKED_PAIRS && P.format != VK_FMT_R8_UNORM) ? VK_LAYOUT_PACKED : vol_layout;
        for (int a = 0; a < 3; a++)
            if (P.n[a] > 8192u) return "VK_RESAMPLE_INSTALL: a volume's extents are at most 8192";
        if (P.layout == VK_LAYOUT_PACKED_PAIRS && P.format != VK_FMT_R8_UNORM) return "VK_RESAMPLE_INSTALL: PACKED_PAIRS stores exact u8 differences; an R16_UNORM or R16_FLOAT output uses PACKED or LINEAR";
        if (P.format == VK_FMT_R16_UNORM && P.layout != VK_LAYOUT_LINEAR && P.layout != VK_LAYOUT_PACKED)
            return "VK_RESAMPLE_INSTALL: R16_UNORM volumes use VK_LAYOUT_LINEAR or VK_LAYOUT_PACKED";
    }
    return nullptr;
}

// ---- the grid -------------------------------------------------------------------------------------------------------------------------
// A 256-thread workgroup owns a tile of 64 x 4 output voxels of one z: lanes along x.  Up to kResampleGrid3dTiles tiles the grid is
// three-dimensional, a block per tile: the tile's place is the block's index and costs no divide.  Beyond that, or under a cap
// (vk_debug_set_param "resample_max_blocks"), the grid is flat: a block takes tiles blockIdx.x + t * blocks, t = 0 .. trips - 1 -- the
// trip count is the launch's, the same for every block; a tile index at or above `tiles` is skipped.
// A thread takes tz output voxels one above the other (resample_tile_z): their loads are independent and in flight together.
constexpr uint32_t kResampleThreads = 256, kResampleTileX = 64, kResampleTileY = 4;
// the tile's depth: 4, but 1 where a voxel alone keeps many loads in flight or loops over its taps (AREA other than the unrolled ratio 2)
constexpr uint32_t resample_tile_z(int mode, uint32_t unrolled_taps) { return (mode == VK_RESAMPLE_AREA && unrolled_taps != 2u) ? 1u : 4u; }
constexpr uint32_t kResampleMaxBlocks = 1u << 22;
constexpr uint64_t kResampleGrid3dTiles = 1ull << 23;  // 2^31 threads
struct ResampleGrid {
    uint32_t ntx, nty, ntz, blocks;  // flat: blocks; otherwise the grid is ntx x nty x ntz
    uint32_t flat;
    uint64_t tiles, trips;
};
inline ResampleGrid resample_grid(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t max_blocks, uint32_t tz = 1u) {
    ResampleGrid G;
    G.ntx = (nx + kResampleTileX - 1u) / kResampleTileX;
    G.nty = (ny + kResampleTileY - 1u) / kResampleTileY;
    G.ntz = (nz + tz - 1u) / tz;
    G.tiles = (uint64_t)G.ntx * G.nty * G.ntz;
    G.flat = (max_blocks || G.tiles > kResampleGrid3dTiles) ? 1u : 0u;
    uint64_t b = G.tiles > kResampleMaxBlocks ? kResampleMaxBlocks : G.tiles;
    if (max_blocks && b > max_blocks) b = max_blocks;
    G.blocks = b < 1u ? 1u : (uint32_t)b;
    G.trips = G.flat ? (G.tiles + G.blocks - 1u) / G.blocks : 1u;
    return G;
}

}  // namespace vk
