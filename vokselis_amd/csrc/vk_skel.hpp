// vk_skel.hpp -- skeleton of a value range (vk_skeletonize): the validation of a caller's vk_skeleton_request in
// its order, the neighbourhood mask's bit order, the simple-point test, the class of a voxel, the state byte and the mapping of a
// workgroup's threads onto a tile's voxels of one subfield, for the kernels and their host (vk_launch_skel.hip); plain C++ that g++
// compiles without a device, as vk_geo.hpp is, so that the host fuzz (tests/skel_fuzz.cpp) shares it.  The range predicate, the
// neighbour offsets, the box test, the tile and the fill rule are the label pass's (vk_label.hpp); the window of a tile with its
// one-voxel halo, the tile of a voxel and a tile's neighbours are the geodesic pass's (vk_geo.hpp), bytes here where they are words there.
//
// The state byte.  One per voxel: 0 background (off S, or deleted in an iteration before the last), 1 in K, kSkelGone + (i & 1) deleted
// in iteration i.  In iteration i a voxel "is in K" iff its byte is 1 and "was in K_i" iff its byte is 1 or kSkelGone + (i & 1); the
// byte of the other parity means background and is set to 0 by the workgroup that owns it when it next visits the voxel's sub-pass --
// it does in iteration i + 1, because a tile that deletes a voxel stamps itself -- so that no such byte is left when iteration i + 2
// writes that value again.  Both readings are the same before and after that store, so no reader cares which it sees.
#pragma once

#include "vk_geo.hpp"
#include "vk_label.hpp"

namespace vk {

// ---- the request -------------------------------------------------------------------------------------------------------------
// A caller's request without the volume (the box and the volume's kind are the entry point's).  Returns nullptr, or what is wrong
// (VK_ERR_INVALID): the first of the header's list that applies.
inline const char *skel_validate(const vk_skeleton_request *r, bool have_class, bool have_dense, bool have_result) {
    if (!r) return "the request is NULL";
    if (isnan(r->lo) || isnan(r->hi)) return "lo or hi is NaN";
    if (r->lo > r->hi) return "lo > hi";
    if (r->mode != (uint32_t)VK_SKEL_CURVE && r->mode != (uint32_t)VK_SKEL_KERNEL) return "unknown mode (VK_SKEL_CURVE, VK_SKEL_KERNEL)";
    if (r->flags & ~(uint32_t)(VK_SKEL_CLIP_BOX | VK_SKEL_INSTALL | VK_SKEL_FILL_IN)) return "unknown flag (VK_SKEL_CLIP_BOX, VK_SKEL_INSTALL, VK_SKEL_FILL_IN)";
    if (r->pad != 0u) return "pad must be 0";
    if (!isfinite(r->fill_out)) return "fill_out is not finite";
    if ((r->flags & VK_SKEL_FILL_IN) && !isfinite(r->fill_in)) return "fill_in is not finite under VK_SKEL_FILL_IN";
    if (!have_class && !have_dense && !have_result && !(r->flags & VK_SKEL_INSTALL)) return "none of class_out, dense_out, VK_SKEL_INSTALL and result: the result would go nowhere";
    return nullptr;
}

// ---- the neighbourhood ---------------------------------------------------------------------------------------------------------
// Two forms of one mask.  The caller's m has 26 bits: bit k is the neighbour at label_offset(k < 13 ? k : k + 1).  The form the test
// works on, m27, has bit o for label_offset(o) -- o = x + 3 y + 9 z over x, y, z = 0 .. 2 -- and its centre bit clear, so that a step
// along an axis is a shift.
constexpr uint32_t kSkelBits = 26, kSkelAll27 = (1u << kLabelOffsets) - 1u, kSkelLow = (1u << kLabelCentre) - 1u;
VK_LABEL_HD uint32_t skel_mask_offset(uint32_t k) { return k < kLabelCentre ? k : k + 1u; }
VK_LABEL_HD uint32_t skel_expand(uint32_t m) { return (m & kSkelLow) | ((m >> kLabelCentre) << (kLabelCentre + 1u)); }
VK_LABEL_HD uint32_t skel_compress(uint32_t m27) { return (m27 & kSkelLow) | ((m27 >> (kLabelCentre + 1u)) << kLabelCentre); }
// the positions whose coordinate on axis a (stride 1, 3, 9) is c
constexpr uint32_t skel_plane(uint32_t stride, uint32_t c) {
    uint32_t m = 0u;
    for (uint32_t o = 0; o < kLabelOffsets; o++)
        if (o / stride % 3u == c) m |= 1u << o;
    return m;
}
// the positions with |d|_1 in [lo, hi]
constexpr uint32_t skel_shell(uint32_t lo, uint32_t hi) {
    uint32_t m = 0u;
    for (uint32_t o = 0; o < kLabelOffsets; o++) {
        const uint32_t s = (o % 3u != 1u) + (o / 3u % 3u != 1u) + (o / 9u != 1u);
        if (s >= lo && s <= hi) m |= 1u << o;
    }
    return m;
}
constexpr uint32_t kSkelX0 = skel_plane(1u, 0u), kSkelX2 = skel_plane(1u, 2u), kSkelY0 = skel_plane(3u, 0u), kSkelY2 = skel_plane(3u, 2u);
constexpr uint32_t kSkelFaces = skel_shell(1u, 1u), kSkelEighteen = skel_shell(1u, 2u);
static_assert(kSkelX0 == 0x1249249u && kSkelY0 == 0x1C0E07u && kSkelFaces == ((1u << 4) | (1u << 10) | (1u << 12) | (1u << 14) | (1u << 16) | (1u << 22)), "the planes and the faces of the 3 x 3 x 3 positions");

// one step of c along +-x, +-y, +-z inside the 3 x 3 x 3 positions: a shift, without what would leave a row, a plane or the cube
VK_LABEL_HD uint32_t skel_step_x(uint32_t c) { return ((c << 1) & (kSkelAll27 & ~kSkelX0)) | ((c >> 1) & ~kSkelX2); }
VK_LABEL_HD uint32_t skel_step_y(uint32_t c) { return ((c << 3) & (kSkelAll27 & ~kSkelY0)) | ((c >> 3) & ~kSkelY2); }
VK_LABEL_HD uint32_t skel_step_z(uint32_t c) { return ((c << 9) & kSkelAll27) | (c >> 9); }

// The simple-point test on m27 (centre bit clear).  Two floods from one bit each, every trip one dilation of the whole front by shifts:
// (a) over the set bits by 26-adjacency -- the dilation along x, then y, then z reaches the 3 x 3 x 3 cube around every bit --, (b) over
// the clear bits of the 18 positions by 6-adjacency.  A flood ends when a trip adds nothing; every trip before adds a bit, so there
// are at most 26 and 18.  (a) holds iff the flood from the lowest set bit is all of m27; (b) iff a clear face exists and the flood
// from the lowest clear face holds every clear face.
VK_LABEL_HD bool skel_simple27(uint32_t m27) {
    if (m27 == 0u) return false;
    uint32_t c = m27 & (0u - m27);
    for (uint32_t trip = 0; trip < kSkelBits; trip++) {
        uint32_t d = c | skel_step_x(c);
        d |= skel_step_y(d);
        d |= skel_step_z(d);
        d &= m27;
        if (d == c) break;
        c = d;
    }
    if (c != m27) return false;
    const uint32_t open = ~m27 & kSkelEighteen, faces = open & kSkelFaces;
    if (faces == 0u) return false;
    c = faces & (0u - faces);
    for (uint32_t trip = 0; trip < 18u; trip++) {
        const uint32_t d = (c | skel_step_x(c) | skel_step_y(c) | skel_step_z(c)) & open;
        if (d == c) break;
        c = d;
    }
    return (faces & ~c) == 0u;
}
VK_LABEL_HD bool skel_simple(uint32_t m) { return skel_simple27(skel_expand(m)); }
VK_LABEL_HD uint32_t skel_popcount(uint32_t m) {
    uint32_t n = 0u;
    for (; m; m &= m - 1u) n++;
    return n;
}
VK_LABEL_HD bool skel_line_end(uint32_t m) { return m != 0u && (m & (m - 1u)) == 0u; }
// the class of a voxel: VK_SKEL_OFF off K, else by its neighbours in K
VK_LABEL_HD uint32_t skel_class(bool in_k, uint32_t neighbours) {
    return !in_k ? (uint32_t)VK_SKEL_OFF : (neighbours >= 3u ? (uint32_t)VK_SKEL_JUNCTION : (uint32_t)VK_SKEL_ISOLATED + neighbours);
}
VK_LABEL_HD uint32_t skel_subfield(uint32_t x, uint32_t y, uint32_t z) { return (x & 1u) | ((y & 1u) << 1) | ((z & 1u) << 2); }

// ---- the state byte ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t kSkelOff = 0u, kSkelIn = 1u, kSkelGone = 2u;
VK_LABEL_HD uint32_t skel_gone(uint32_t iteration) { return kSkelGone + (iteration & 1u); }
VK_LABEL_HD bool skel_in(uint32_t state) { return state == kSkelIn; }
VK_LABEL_HD bool skel_was_in(uint32_t state, uint32_t iteration) { return state == kSkelIn || state == skel_gone(iteration); }

// What sub-pass s of iteration `iteration` does to voxel (wx, wy, wz) of a window of kGeoWinX x kGeoWinY x kGeoWinZ state bytes (a tile
// and its halo, 0 outside the volume; the voxel is the tile's, so every neighbour is a cell of the window): the byte it stores, or the
// byte it found where it stores nothing.  L: L::load(p, i).  The window is read as it is found: every cell this reads belongs to
// another subfield than the voxel's, and no voxel of another subfield changes during the sub-pass.
template <class L, class P>
VK_LABEL_HD uint32_t skel_visit(P win, uint32_t wx, uint32_t wy, uint32_t wz, uint32_t iteration, bool curve) {
    const uint32_t c = geo_window_index(wx, wy, wz);
    const uint32_t st = L::load(win, c);
    if (st == skel_gone(iteration + 1u)) return kSkelOff;  // deleted in the iteration before: background from now on
    if (st != kSkelIn) return st;
    uint32_t m27 = 0u, was = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t o = 0; o < kLabelOffsets; o++) {
        if (o == kLabelCentre) continue;
        int dx, dy, dz;
        label_offset(o, dx, dy, dz);
        const uint32_t nb = L::load(win, (uint32_t)((int)c + dx + (int)kGeoWinX * (dy + (int)kGeoWinY * dz)));
        m27 |= skel_in(nb) ? 1u << o : 0u;
        was |= skel_was_in(nb, iteration) ? 1u << o : 0u;
    }
    if ((was & kSkelFaces) == kSkelFaces) return st;                       // not a candidate: all six face neighbours were in K_i
    if (curve && skel_line_end(m27)) return st;
    return skel_simple27(m27) ? skel_gone(iteration) : st;
}

// ---- a tile's voxels of one subfield -------------------------------------------------------------------------------------------------
// A tile's origin is even on every axis, so a voxel's subfield is that of its local coordinates: 512 of the 4096 voxels, two per
// thread.  Voxel j = 0 .. 511 of subfield s, x fastest.
constexpr uint32_t kSkelSubVoxels = kLabelTileVoxels / 8u, kSkelPerThread = kSkelSubVoxels / kLabelThreads;
static_assert(kLabelTile.tx % 2u == 0 && kLabelTile.ty % 2u == 0 && kLabelTile.tz % 2u == 0 && kSkelSubVoxels % kLabelThreads == 0, "a tile's origin is even; its voxels of a subfield are a multiple of the workgroup");
VK_LABEL_HD void skel_sub_coords(uint32_t j, uint32_t s, uint32_t &lx, uint32_t &ly, uint32_t &lz) {
    constexpr uint32_t hx = kLabelTile.tx / 2u, hy = kLabelTile.ty / 2u;
    lx = 2u * (j % hx) + (s & 1u);
    ly = 2u * (j / hx % hy) + ((s >> 1) & 1u);
    lz = 2u * (j / (hx * hy)) + ((s >> 2) & 1u);
}
constexpr uint32_t kSkelAllTiles = kSkelAll27;  // the tile itself and its 26 neighbours: what a tile that deleted a voxel stamps
// Why that stamp suffices.  A tile runs in iteration i + 1 iff it or a tile around it deleted a voxel in iteration i.  A voxel w of a
// tile T that does not run in iteration i + 1 would be deleted there only behind a chain of deletions of that same iteration, each in a
// later sub-pass than the one before and each within one voxel of the next, whose first link was made deletable by a change of iteration
// i: a chain has at most eight links, w included, so that change lies within eight voxels of T -- inside T or a tile around it, as no
// tile extent is below eight -- and would have stamped T.
static_assert(kLabelTile.tx >= 8u && kLabelTile.ty >= 8u && kLabelTile.tz >= 8u, "a chain of one iteration's eight sub-passes stays inside the tiles around a tile");

// How many iterations (of eight launches) the host enqueues between two looks at the iterations' counts.  An iteration that deletes
// nothing stamps no tile: the iterations behind it in the batch find no active tile and change nothing.
constexpr uint32_t kSkelBatch = 4;
constexpr uint32_t kSkelIterWords = 2;  // per iteration: voxels deleted, tile visits

}  // namespace vk
