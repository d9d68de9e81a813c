// vk_shadow.hpp -- light-direction shadows of the first-hit isosurface march (vk_set_shadows): the descriptor the
// shadow kernels read, the host validation, and the two host-callable pieces of the shade -- the first shadow sample's distance ts0 and
// the factor k -- shared by the kernels (vk_launch_iso_shadow.hip, vk_launch_u16_iso_shadow.hip), the host (vk_render.hip) and the host
// fuzz (tests/shadow_fuzz.cpp, plain g++ under ASan / UBSan).
//
// A ray that hit casts one more isosurface ray from its refined crossing q along the unit light direction L, through the box the
// primary ray marched, every operation one f32 rounding:
//   dts = dt_scale * min(1 / (nx |L.x|), 1 / (ny |L.y|), 1 / (nz |L.z|))       the primary ray's dt with L for dir
//   intersect_box(q, L, lo, hi) -> tb0, tb1;  tb0 > tb1: not shadowed
//   ts0 = max(max(tb0, 0), bias * dts);  ps = fma(ts0, L, q);  ss = L * dts
//   for (t = ts0; t < tb1; t = t + dts) { if (trilinear(V, ps) >= iso_k) shadowed; ps = ps + ss }
//   k = shadowed ? 1 - strength : 1;  rgb' = c.rgb * (ka + kd * diff * k) + ks * spec * k
// The loops are the isosurface's (vk_march_iso.hpp), called a second time from the kernel body's epilogue with the integer trip budget of
// vk_trips.hpp; the shadow ray counts in neither the step image nor the counters.
//
// Why skipping stays exact.  The shadow ray's operator is the primary ray's, x >= iso_k on the same filter, so the emptiness predicate of
// a cell is the same (vk_iso.hpp: iso_cell_empty) and the skip maps built for the isosurface, one per octant, hold for any direction: a
// skipped shadow step lies in a cell whose samples all stay below iso_k, it would not have hit, and the walk advances ps by the
// reference's own additions.  A shadow ray carries nothing else from one step to the next.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VK_SHADOW_HD __host__ __device__ __forceinline__
#else
#define VK_SHADOW_HD inline
#endif

namespace vk {

constexpr float kShadowMaxBias = 1024.0f;  // VK_SHADOW_MAX_BIAS

// What the shadow kernels read (a kernel argument of their own, beside IsoDesc).
struct ShadowDesc {
    float k;     // 1 - strength: what a shadowed point keeps of its diffuse and specular terms
    float bias;  // the first shadow sample's distance from the surface, in shadow steps
};
static_assert(sizeof(ShadowDesc) == 8, "ShadowDesc: two words");

// The factor of a shadowed point.
VK_SHADOW_HD float shadow_k(float strength) { return 1.0f - strength; }

// Where the shadow ray starts: at the box's entry (never behind q) and at least `bias` shadow steps from the surface.
VK_SHADOW_HD float shadow_ts0(float tb0, float bias, float dts) { return fmaxf(fmaxf(tb0, 0.0f), bias * dts); }

// Host validation of the public parameters (vk_shadows' fields); fills the descriptor and returns nullptr, or returns what is wrong.
inline const char *shadow_desc(float strength, float bias, ShadowDesc &D) {
    if (!isfinite(strength) || !isfinite(bias)) return "a field is not finite";
    if (!(strength >= 0.0f && strength <= 1.0f)) return "strength must lie in [0, 1]";
    if (!(bias >= 0.0f && bias <= kShadowMaxBias)) return "bias must lie in [0, VK_SHADOW_MAX_BIAS]";
    D.k = shadow_k(strength);
    D.bias = bias + 0.0f;  // (a -0 is stored as +0)
    return nullptr;
}

}  // namespace vk
