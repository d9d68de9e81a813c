// vk_split.hpp -- split touching objects (vk_split_components): the validation of a caller's vk_split_request, the
// states of the growth array and one voxel's step of a growth round, for the kernels and their host (vk_launch_split.hip); plain C++ that
// g++ compiles without a device, as vk_label.hpp and vk_dist.hpp are, so that a host fuzz can share it.  The predicate, the neighbour offsets, the union-find and the tile, seam
// and chunk arithmetic are the label pass's (vk_label.hpp); R2 and the overflow bound are the distance pass's (vk_dist.hpp).
//
// The state array.  One word per voxel: the anchor a(v) of a voxel a marker has reached (a linear index, <= kLabelMaxVoxels - 1), or
// kSplitUnreached for a voxel of S that no marker has reached yet, or kLabelBackground off S.  The three kinds are ordered
//     anchor < kSplitUnreached < kLabelBackground,
// so the minimum over a voxel's neighbours is the smallest anchor among them where one exists and is >= kSplitUnreached otherwise.
#pragma once

#include "vk_dist.hpp"
#include "vk_label.hpp"

namespace vk {

constexpr uint32_t kSplitUnreached = 0xfffffffeu;
static_assert(kLabelMaxVoxels - 1u < kSplitUnreached && kSplitUnreached < kLabelBackground, "an anchor is a voxel index: below both marks");

// ---- the request -------------------------------------------------------------------------------------------------------------
// A caller's request without the volume (the box, the volume's kind, the overflow bound and the fill against the range are the entry
// point's).  Returns nullptr, or what is wrong (VK_ERR_INVALID).
inline const char *split_validate(const vk_split_request *r, bool have_labels, bool have_components, uint64_t cap_components, bool have_dense, bool have_result) {
    if (!r) return "the request is NULL";
    if (isnan(r->lo) || isnan(r->hi)) return "lo or hi is NaN";
    if (r->lo > r->hi) return "lo > hi";
    if (r->connectivity != 6u && r->connectivity != 18u && r->connectivity != 26u) return "connectivity must be 6, 18 or 26";
    if (r->flags & ~(uint32_t)(VK_SPLIT_CLIP_BOX | VK_SPLIT_INSTALL)) return "unknown flag (VK_SPLIT_CLIP_BOX, VK_SPLIT_INSTALL)";
    if (r->pad != 0u) return "pad must be 0";
    for (int c = 0; c < 3; c++)
        if (r->spacing[c] < 1u || r->spacing[c] > (uint32_t)VK_DIST_MAX_SPACING) return "a spacing outside 1 .. VK_DIST_MAX_SPACING";
    if (!isfinite(r->radius) || r->radius < 0.0f || r->radius > VK_DIST_MAX_RADIUS) return "the radius is not finite, is negative or lies above VK_DIST_MAX_RADIUS";
    if (!isfinite(r->fill_out)) return "fill_out is not finite";
    if (have_components && cap_components == 0u) return "components with cap_components == 0";
    if (!have_labels && !have_components && !have_dense && !have_result && !(r->flags & VK_SPLIT_INSTALL))
        return "none of labels_out, components, dense_out, VK_SPLIT_INSTALL and result: the result would go nowhere";
    return nullptr;
}

// the value of a half's bits (host: the validation alone)
inline float split_half_value(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    const float v = e == 31u ? (m ? NAN : INFINITY) : (e == 0u ? ldexpf((float)m, -24) : ldexpf((float)(m | 1024u), (int)e - 25));
    return (h & 0x8000u) ? -v : v;
}
// Whether a cut voxel leaves S: F(fill_out), as a stored texel on the kernel's scale, lies outside [lo_k, hi_k].
inline bool split_fill_leaves_set(float fill_out, int format, float lo_k, float hi_k) {
    const uint32_t bits = label_fill_bits(fill_out, format);
    const float t = format == VK_FMT_R16_FLOAT ? split_half_value(bits) : (float)bits;
    return !label_foreground(t, lo_k, hi_k);
}

// ---- a round of the growth -----------------------------------------------------------------------------------------------------
// What voxel (x, y, z), whose state in `in` is kSplitUnreached, holds after this round: the smallest state among its neighbours in `in`
// -- the smallest anchor that round k - 1 or an earlier one left beside it -- or kSplitUnreached when none of them has one.  `in` is the
// state after the round before and is only read: a voxel labelled in this round goes to the other array and is seen by no neighbour
// before the next launch, which is what makes g(v) the length of the shortest path and a(v) the minimum over g(u) = g(v) - 1 alone.
// L: L::load(in, i).
template <class L, class P>
VK_LABEL_HD uint32_t split_grow_voxel(P in, uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t conn_sum) {
    uint32_t best = kSplitUnreached;
    for (uint32_t o = 0; o < kLabelOffsets; o++) {
        int dx, dy, dz;
        label_offset(o, dx, dy, dz);
        if (!label_adjacent(dx, dy, dz, conn_sum)) continue;
        const int64_t hx = (int64_t)x + dx, hy = (int64_t)y + dy, hz = (int64_t)z + dz;  // no wrap: a neighbour outside the volume does not exist
        if (hx < 0 || hy < 0 || hz < 0 || hx >= (int64_t)nx || hy >= (int64_t)ny || hz >= (int64_t)nz) continue;
        const uint32_t s = L::load(in, (uint32_t)voxel_index((uint32_t)hx, (uint32_t)hy, (uint32_t)hz, nx, ny));
        best = s < best ? s : best;
    }
    return best;
}

// How many rounds the host launches between two looks at the rounds' counts.  A round that labels nothing leaves the state as it
// found it and so does every round after it: the rounds past the last one that labelled a voxel change nothing and are not counted.
constexpr uint32_t kSplitBatch = 8;

}  // namespace vk
