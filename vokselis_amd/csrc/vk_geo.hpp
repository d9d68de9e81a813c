// vk_geo.hpp -- geodesic distance through a value range (vk_geodesic_distance): the validation of a caller's
// vk_geodesic_request in its order, the step costs, the saturating relaxation, the face predicate, one voxel's relaxation over its
// neighbours and the tile and halo arithmetic, for the kernels and their host (vk_launch_geo.hip); plain C++ that g++ compiles without a
// device, as vk_split.hpp is, so that the host fuzz (tests/geo_fuzz.cpp) shares it.  The range predicate, the neighbour offsets,
// label_adjacent, the box test, the tile and the fill rule are the label pass's (vk_label.hpp).
//
// The state array.  One word per voxel: g so far -- 0 on a source, the length of some path from a source on a voxel a front has
// reached, VK_GEO_INF on every other voxel, off S included.  A word only ever decreases, and every value it holds is the length of a
// real path inside S (saturated at VK_GEO_FAR): a reader that sees an older value relaxes from a longer real path, which gives an upper
// bound of the fixed point, never something below it.
#pragma once

#include "vk_dist.hpp"
#include "vk_label.hpp"

namespace vk {

constexpr uint32_t kGeoInf = VK_GEO_INF, kGeoFar = VK_GEO_FAR;
constexpr uint32_t kGeoFaceMask = 63u;

// ---- the request -------------------------------------------------------------------------------------------------------------
// A caller's request without the volume (the seeds against the volume, the box and the volume's kind are the entry point's).  Returns
// nullptr, or what is wrong (VK_ERR_INVALID): the first of the header's list that applies.
inline const char *geo_validate(const vk_geodesic_request *r, bool have_g, bool have_dense, bool have_result) {
    if (!r) return "the request is NULL";
    if (isnan(r->lo) || isnan(r->hi)) return "lo or hi is NaN";
    if (r->lo > r->hi) return "lo > hi";
    if (r->connectivity != 6u && r->connectivity != 18u && r->connectivity != 26u) return "connectivity must be 6, 18 or 26";
    if (r->flags & ~(uint32_t)(VK_GEO_CLIP_BOX | VK_GEO_INSTALL)) return "unknown flag (VK_GEO_CLIP_BOX, VK_GEO_INSTALL)";
    if (r->pad != 0u) return "pad must be 0";
    for (int c = 0; c < 3; c++)
        if (r->spacing[c] < 1u || r->spacing[c] > (uint32_t)VK_DIST_MAX_SPACING) return "a spacing outside 1 .. VK_DIST_MAX_SPACING";
    if ((r->source_faces | r->target_faces) & ~kGeoFaceMask) return "a face mask with a bit above VK_GEO_FACE_Z1";
    if (r->n_seeds > (uint32_t)VK_GEO_MAX_SEEDS) return "n_seeds above VK_GEO_MAX_SEEDS";
    if (r->source_faces == 0u && r->n_seeds == 0u) return "no source: source_faces is 0 and n_seeds is 0";
    if (!isfinite(r->gain) || r->gain < 0.0f) return "gain is negative or not finite";
    if (!isfinite(r->fill_out) || !isfinite(r->fill_unreached)) return "fill_out or fill_unreached is not finite";
    if (!have_g && !have_dense && !have_result && !(r->flags & VK_GEO_INSTALL)) return "none of g_out, dense_out, VK_GEO_INSTALL and result: the result would go nowhere";
    return nullptr;
}
inline bool geo_seeds_inside(const vk_geodesic_request *r, uint32_t nx, uint32_t ny, uint32_t nz) {
    for (uint32_t s = 0; s < r->n_seeds; s++)
        if (r->seeds[s][0] >= nx || r->seeds[s][1] >= ny || r->seeds[s][2] >= nz) return false;
    return true;
}
// the automatic gain
inline float geo_auto_gain(uint32_t max_g) { return max_g ? 1.0f / (float)max_g : 0.0f; }

// ---- step costs ----------------------------------------------------------------------------------------------------------------
// w(d): the largest r with r r <= 65536 q(d), q(d) = sum_c (spacing[c] d_c)^2 <= 3 * 64^2 = 12288, so 65536 q < 2^30 and r < 2^15.
// One bit of r per trip from the top, integers only.
VK_DIST_HD uint32_t geo_weight(const uint32_t spacing[3], int dx, int dy, int dz) {
    const int64_t ex = (int64_t)spacing[0] * dx, ey = (int64_t)spacing[1] * dy, ez = (int64_t)spacing[2] * dz;
    const uint64_t q = (uint64_t)(ex * ex + ey * ey + ez * ez) << 16;
    uint32_t r = 0u;
    for (uint32_t bit = 1u << 15; bit; bit >>= 1) {
        const uint64_t t = (uint64_t)(r | bit);
        if (t * t <= q) r |= bit;
    }
    return r;
}
// w[o] for the offsets o of label_offset: the cost of an adjacent offset, 0 elsewhere (the centre; an offset the connectivity leaves out)
struct GeoWeights { uint32_t w[kLabelOffsets]; };
VK_DIST_HD GeoWeights geo_weights(const uint32_t spacing[3], uint32_t conn_sum) {
    GeoWeights W;
    for (uint32_t o = 0; o < kLabelOffsets; o++) {
        int dx, dy, dz;
        label_offset(o, dx, dy, dz);
        W.w[o] = label_adjacent(dx, dy, dz, conn_sum) ? geo_weight(spacing, dx, dy, dz) : 0u;
    }
    return W;
}
// The saturating step from a finite a: min(a + w, VK_GEO_FAR).  a <= VK_GEO_FAR, so the room below VK_GEO_FAR is no wrap, and the sum
// is formed only where it fits: 32-bit arithmetic throughout, and VK_GEO_INF never comes out.
VK_DIST_HD uint32_t geo_relax(uint32_t a, uint32_t w) {
    const uint32_t room = kGeoFar - a;
    return w < room ? a + w : kGeoFar;
}

// ---- faces ---------------------------------------------------------------------------------------------------------------------
// Whether voxel (x, y, z) of the non-empty box b lies on one of the faces of `mask`: its coordinate is b's first or last index there.
VK_DIST_HD bool geo_on_faces(uint32_t x, uint32_t y, uint32_t z, const vk_voxel_box &b, uint32_t mask) {
    uint32_t on = 0u;
    on |= x == b.x0 ? (uint32_t)VK_GEO_FACE_X0 : 0u;
    on |= x + 1u == b.x1 ? (uint32_t)VK_GEO_FACE_X1 : 0u;
    on |= y == b.y0 ? (uint32_t)VK_GEO_FACE_Y0 : 0u;
    on |= y + 1u == b.y1 ? (uint32_t)VK_GEO_FACE_Y1 : 0u;
    on |= z == b.z0 ? (uint32_t)VK_GEO_FACE_Z0 : 0u;
    on |= z + 1u == b.z1 ? (uint32_t)VK_GEO_FACE_Z1 : 0u;
    return (on & mask) != 0u;
}

// ---- one voxel's relaxation ------------------------------------------------------------------------------------------------------
// What voxel (x, y, z) of an array of nx x ny x nz words, x fastest, may be lowered to: the smallest geo_relax(g(u), w) over its adjacent
// u inside the array with a finite g(u), or `cur`, its own word, where none is smaller.  The caller holds that the voxel is in S; a
// neighbour off S holds VK_GEO_INF and gives nothing.  The array is read as it is found -- the caller may be lowering other words of it
// meanwhile (see the head of this file).  L: L::load(p, i).  CONN_SUM is a template parameter so that the set of neighbours is known
// where the loop is unrolled: the words are all loaded first, with no branch between the loads, and reduced afterwards -- on the device
// the LDS loads of a voxel are in flight together instead of one behind the other.
template <class L, uint32_t CONN_SUM, class P>
VK_LABEL_HD uint32_t geo_relax_voxel(P p, uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny, uint32_t nz, const GeoWeights &W, uint32_t cur) {
    uint32_t a[kLabelOffsets];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t o = 0; o < kLabelOffsets; o++) {
        int dx, dy, dz;
        label_offset(o, dx, dy, dz);
        a[o] = kGeoInf;
        if (!label_adjacent(dx, dy, dz, CONN_SUM)) continue;
        const int64_t hx = (int64_t)x + dx, hy = (int64_t)y + dy, hz = (int64_t)z + dz;  // no wrap: a neighbour outside the array does not exist
        if (hx < 0 || hy < 0 || hz < 0 || hx >= (int64_t)nx || hy >= (int64_t)ny || hz >= (int64_t)nz) continue;
        a[o] = L::load(p, (uint32_t)voxel_index((uint32_t)hx, (uint32_t)hy, (uint32_t)hz, nx, ny));
    }
    uint32_t best = cur;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t o = 0; o < kLabelOffsets; o++) {
        int dx, dy, dz;
        label_offset(o, dx, dy, dz);
        if (!label_adjacent(dx, dy, dz, CONN_SUM)) continue;
        const uint32_t s = a[o] == kGeoInf ? kGeoInf : geo_relax(a[o], W.w[o]);
        best = s < best ? s : best;
    }
    return best;
}
// ... with the connectivity as a value: conn_sum 1, 2 or 3
template <class L, class P>
VK_LABEL_HD uint32_t geo_relax_voxel_any(P p, uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t conn_sum, const GeoWeights &W, uint32_t cur) {
    return conn_sum == 1u ? geo_relax_voxel<L, 1u>(p, x, y, z, nx, ny, nz, W, cur)
                          : (conn_sum == 2u ? geo_relax_voxel<L, 2u>(p, x, y, z, nx, ny, nz, W, cur) : geo_relax_voxel<L, 3u>(p, x, y, z, nx, ny, nz, W, cur));
}

// ---- tiles and halos -------------------------------------------------------------------------------------------------------------
// A workgroup owns a tile of the label pass's shape, 32 x 16 x 8 voxels, 16 per thread, and relaxes it in LDS inside a window that adds
// one voxel on every side: (32 + 2) x (16 + 2) x (8 + 2) words.  Window cell (wx, wy, wz) is voxel (x0 + wx - 1, y0 + wy - 1, z0 + wz - 1)
// of the tile whose origin is (x0, y0, z0); a cell outside the volume holds VK_GEO_INF.
constexpr uint32_t kGeoWinX = kLabelTile.tx + 2u, kGeoWinY = kLabelTile.ty + 2u, kGeoWinZ = kLabelTile.tz + 2u;
constexpr uint32_t kGeoWindow = kGeoWinX * kGeoWinY * kGeoWinZ;                                  // 6120 words, 24480 bytes
constexpr uint32_t kGeoHalo = kGeoWindow - kLabelTileVoxels;                                     // 2024 cells around the tile
constexpr uint32_t kGeoWinPerThread = (kGeoWindow + kLabelThreads - 1u) / kLabelThreads;         // 24
VK_LABEL_HD uint32_t geo_window_index(uint32_t wx, uint32_t wy, uint32_t wz) { return wx + kGeoWinX * (wy + kGeoWinY * wz); }
VK_LABEL_HD void geo_window_coords(uint32_t c, uint32_t &wx, uint32_t &wy, uint32_t &wz) {
    wx = c % kGeoWinX;
    wy = c / kGeoWinX % kGeoWinY;
    wz = c / (kGeoWinX * kGeoWinY);
}
// the tile of a voxel, and a tile's number from its three
VK_LABEL_HD uint32_t geo_tile_of(uint32_t x, uint32_t y, uint32_t z, uint32_t ntx, uint32_t nty) {
    return x / kLabelTile.tx + ntx * (y / kLabelTile.ty + nty * (z / kLabelTile.tz));
}
// Direction k = 0 .. 26 of the 3 x 3 x 3 tiles around a tile, numbered as label_offset numbers voxels.  The directions a lowered voxel
// (lx, ly, lz) of a tile has to wake, as a mask of 27 bits: every tile other than its own that holds a voxel adjacent to it.  Along an
// axis the voxel faces the tile before when its local coordinate is 0 and the tile after when it is the tile's last; a direction is
// every choice of "stay or cross" over the axes it faces, at most conn_sum crossings at once, at least one.  Whether the tile in that
// direction exists is the caller's question (geo_tile_neighbour).
VK_LABEL_HD uint32_t geo_wake_mask(uint32_t lx, uint32_t ly, uint32_t lz, uint32_t conn_sum) {
    const int sx = lx == 0u ? -1 : (lx == kLabelTile.tx - 1u ? 1 : 0);
    const int sy = ly == 0u ? -1 : (ly == kLabelTile.ty - 1u ? 1 : 0);
    const int sz = lz == 0u ? -1 : (lz == kLabelTile.tz - 1u ? 1 : 0);
    uint32_t mask = 0u;
    for (uint32_t pick = 1u; pick < 8u; pick++) {
        const int ax = (pick & 1u) ? sx : 0, ay = (pick & 2u) ? sy : 0, az = (pick & 4u) ? sz : 0;
        if (((pick & 1u) && !sx) || ((pick & 2u) && !sy) || ((pick & 4u) && !sz)) continue;
        const uint32_t crossings = (pick & 1u) + ((pick >> 1) & 1u) + ((pick >> 2) & 1u);
        if (crossings > conn_sum) continue;
        mask |= 1u << (uint32_t)((ax + 1) + 3 * (ay + 1) + 9 * (az + 1));
    }
    return mask;
}
// The tile in direction k of tile (tx, ty, tz) of ntx x nty x ntz: true and its number, or false where the volume ends.
VK_LABEL_HD bool geo_tile_neighbour(uint32_t tx, uint32_t ty, uint32_t tz, uint32_t ntx, uint32_t nty, uint32_t ntz, uint32_t k, uint32_t &tile) {
    int dx, dy, dz;
    label_offset(k, dx, dy, dz);
    const int64_t hx = (int64_t)tx + dx, hy = (int64_t)ty + dy, hz = (int64_t)tz + dz;
    if (hx < 0 || hy < 0 || hz < 0 || hx >= (int64_t)ntx || hy >= (int64_t)nty || hz >= (int64_t)ntz) return false;
    tile = (uint32_t)hx + ntx * ((uint32_t)hy + nty * (uint32_t)hz);
    return true;
}

// How many rounds the host launches between two looks at the rounds' counts, as kSplitBatch.  A round that wakes no tile leaves nothing
// to do for the rounds after it: they find no active tile and change nothing.
constexpr uint32_t kGeoBatch = 8;
constexpr uint32_t kGeoRoundWords = 4;  // per round: tiles woken, tiles visited, LDS passes, voxels stored

}  // namespace vk
