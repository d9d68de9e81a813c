// vk_diff.hpp -- steady-state diffusion through a value range (vk_steady_diffusion): the validation of a caller's
// vk_diffusion_request in its order, the weights, the automatic omega, q(), one voxel's update over its six neighbours and the
// convergence predicate, for the kernels and their host (vk_launch_diff.hip); plain C++ that g++ compiles without a
// device, as vk_geo.hpp is, so that the host fuzz (tests/diff_fuzz.cpp) runs the same code.  The range predicate, the box test, the tile
// and the fill rule are the label pass's (vk_label.hpp); the window of a tile and its halo is the geodesic pass's (vk_geo.hpp).
//
// The state array.  One word per voxel: the bits of c(v) on S, VK_DIFF_OFF -- a NaN no update can produce: num and den are finite sums
// of finite terms and den > 0 where a quotient is formed -- on every other voxel.  One array therefore answers both "is the neighbour in
// S" and "what is its value", and no kernel behind the seed touches the volume.
// Everything here is compiled with -ffp-contract=off, on the device and on the host: a * b + c is two roundings wherever it is written.
#pragma once

#include "vk_geo.hpp"
#include "vk_label.hpp"

namespace vk {

constexpr uint32_t kDiffOff = VK_DIFF_OFF;
constexpr float kDiffQClamp = 1048576.0f, kDiffQScale = 1073741824.0f;

VK_LABEL_HD uint32_t diff_bits(float f) { return filter_f32_bits(f); }
VK_LABEL_HD float diff_float(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// ---- the request -------------------------------------------------------------------------------------------------------------
// A caller's request without the volume (the box and the volume's kind are the entry point's).  Returns nullptr, or what is wrong
// (VK_ERR_INVALID): the first of the header's list that applies.
inline const char *diff_validate(const vk_diffusion_request *r, bool have_c, bool have_dense, bool have_result) {
    if (!r) return "the request is NULL";
    if (isnan(r->lo) || isnan(r->hi)) return "lo or hi is NaN";
    if (r->lo > r->hi) return "lo > hi";
    if (r->axis > 2u) return "axis must be 0, 1 or 2";
    if (r->flags & ~(uint32_t)(VK_DIFF_CLIP_BOX | VK_DIFF_INSTALL)) return "unknown flag (VK_DIFF_CLIP_BOX, VK_DIFF_INSTALL)";
    for (int c = 0; c < 3; c++)
        if (r->spacing[c] < 1u || r->spacing[c] > (uint32_t)VK_DIST_MAX_SPACING) return "a spacing outside 1 .. VK_DIST_MAX_SPACING";
    if (r->omega != 0.0f && !(r->omega > 0.0f && r->omega < 2.0f)) return "omega must be 0 (automatic) or lie inside (0, 2)";
    if (r->check_every < 1u || r->check_every > (uint32_t)VK_DIFF_MAX_CHECK_EVERY) return "check_every outside 1 .. VK_DIFF_MAX_CHECK_EVERY";
    if (r->max_sweeps < r->check_every) return "max_sweeps < check_every";
    if (!isfinite(r->delta_tol) || r->delta_tol < 0.0f || !isfinite(r->flux_tol) || r->flux_tol < 0.0f) return "delta_tol or flux_tol is negative or not finite";
    if (!isfinite(r->gain) || !isfinite(r->fill_out)) return "gain or fill_out is not finite";
    if (!have_c && !have_dense && !have_result && !(r->flags & VK_DIFF_INSTALL)) return "none of c_out, dense_out, VK_DIFF_INSTALL and result: the result would go nowhere";
    return nullptr;
}

// ---- weights, omega ------------------------------------------------------------------------------------------------------------
struct DiffWeights { float w[3], g; };
VK_LABEL_HD DiffWeights diff_weights(const uint32_t spacing[3], uint32_t axis) {
    DiffWeights W;
    for (int c = 0; c < 3; c++) W.w[c] = (float)(1.0 / (double)(spacing[c] * spacing[c]));
    W.g = 2.0f * W.w[axis];
    return W;
}
// plain double arithmetic, no libm: the same bits from every implementation
inline float diff_auto_omega(uint32_t n_a) {
    const float w = (float)(2.0 / (1.0 + 3.141592653589793 / (double)((uint64_t)n_a + 1u)));
    return w < 2.0f ? w : 1.99999988079071044921875f;  // n_a above 10^8: the conversion rounds to 2, which is no valid omega
}
inline float diff_omega(const vk_diffusion_request *r, uint32_t n_a) { return r->omega != 0.0f ? r->omega : diff_auto_omega(n_a); }

// ---- q -------------------------------------------------------------------------------------------------------------------------
// (int64_t)(clamp(t) * 2^30): comparisons, not fminf / fmaxf, so that a NaN gives the lower clamp everywhere.  |clamp(t)| <= 2^20: the
// product is exact (a power of two, no overflow, no underflow that matters: a product below 1 truncates to 0 either way) and fits.
VK_LABEL_HD int64_t diff_q(float t) {
    const float k = t >= -kDiffQClamp ? (t <= kDiffQClamp ? t : kDiffQClamp) : -kDiffQClamp;
    return (int64_t)(k * kDiffQScale);
}
VK_LABEL_HD int64_t diff_flux_in_q(float c) { return diff_q(2.0f * (1.0f - c)); }
VK_LABEL_HD int64_t diff_flux_out_q(float c) { return diff_q(2.0f * c); }

// ---- one voxel's update --------------------------------------------------------------------------------------------------------
// The six neighbour words of voxel (x, y, z) of an array of nx x ny x nz state words, x fastest, in the order x-, x+, y-, y+, z-, z+;
// VK_DIFF_OFF for a neighbour outside the array.  L: L::load(p, i), the word at index i.  No load stands behind a branch: where there
// is no neighbour the voxel's own word is loaded and dropped, so that a caller's loads -- of several voxels -- can all be in flight at
// once.
template <class L, class P>
VK_LABEL_HD void diff_load_neighbours(P p, uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t a[6]) {
    const uint64_t i = voxel_index(x, y, z, nx, ny), sy = nx, sz = (uint64_t)nx * ny;
    const bool has[6] = {x > 0u, x + 1u < nx, y > 0u, y + 1u < ny, z > 0u, z + 1u < nz};
    const uint64_t at[6] = {i - 1u, i + 1u, i - sy, i + sy, i - sz, i + sz};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 6u; k++) {
        const uint32_t w = L::load(p, (uint32_t)(has[k] ? at[k] : i));
        a[k] = has[k] ? w : kDiffOff;
    }
}
// c'(v) from the voxel's own value c and its six neighbour words: the header's rule, the words folded in their order, a word
// VK_DIFF_OFF left out.  Returns false where den == 0: the voxel is never updated.
VK_LABEL_HD bool diff_update_from(const uint32_t a[6], const DiffWeights &W, bool inlet, bool outlet, float omega, float c, float &c_new) {
    float num = 0.0f, den = 0.0f;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 6u; k++) {
        if (a[k] == kDiffOff) continue;
        const float w = W.w[k >> 1];
        const float t = w * diff_float(a[k]);
        num = num + t;
        den = den + w;
    }
    if (inlet) { num = num + W.g; den = den + W.g; }
    if (outlet) den = den + W.g;
    if (den == 0.0f) return false;
    const float gs = num / den;
    const float d = gs - c;
    const float step = omega * d;
    c_new = c + step;
    return true;
}
// ... both: the update of voxel (x, y, z) of the array
template <class L, class P>
VK_LABEL_HD bool diff_update_voxel(P p, uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny, uint32_t nz, const DiffWeights &W, bool inlet, bool outlet, float omega, float c,
                                   float &c_new) {
    uint32_t a[6];
    diff_load_neighbours<L>(p, x, y, z, nx, ny, nz, a);
    return diff_update_from(a, W, inlet, outlet, omega, c, c_new);
}

// ---- the stopping rule ---------------------------------------------------------------------------------------------------------
VK_LABEL_HD bool diff_converged(float delta, int64_t fin_q, int64_t fout_q, float delta_tol, float flux_tol) {
    const double fi = (double)fin_q, fo = (double)fout_q;
    const double gap = fi - fo;
    const double mean = 0.5 * (fi + fo);
    return (double)delta <= (double)delta_tol && (gap < 0.0 ? -gap : gap) <= (double)flux_tol * mean;
}

// ---- the rounds ----------------------------------------------------------------------------------------------------------------
// A round of PassCall::iterate is one block of check_every sweeps and its check.  Per round: the bits of delta, Fin_q, Fout_q, whether
// the block converged, whether it ran at all (a round behind the converged one finds the "done" word set and leaves everything alone).
constexpr uint32_t kDiffBatch = 4;
constexpr uint32_t kDiffRoundWords = 6;
enum { kDiffSlotDelta = 0, kDiffSlotFin = 1, kDiffSlotFout = 2, kDiffSlotConverged = 3, kDiffSlotRan = 4 };

}  // namespace vk
