// vk_iso.hpp -- first-hit isosurface rendering of NAIVE_TRILINEAR (vk_set_isosurface): the descriptor the isosurface
// kernels read, the host validation, the threshold on the kernel's scale, the hit test, the emptiness predicate of a cell and the
// refinement of the crossing, shared by the kernels (vk_launch_iso.hip), the skip-map rebuild (vk_volume.hip), the host (vk_render.hip)
// and the host fuzz (tests/iso_fuzz.cpp, plain g++ under ASan / UBSan).
//
// A ray takes the reference's loop; its first sample x with x >= iso_k ends it, with p left at that sample (never advanced past it).
// The crossing lies at most one step back towards the eye: a = 0, then for i = 1 .. R: m = a + 2^-i; q = fma(-m, s, p) per component;
// a = m if the sample at q hits.  a is a dyadic fraction of R bits in [0, 1 - 2^-R], every m exact in f32 (R <= 16).  A hit in a ray's
// first iteration is not refined: there is no sample before it, the surface is the cut face of the box.  The sample at
// q = fma(-a, s, p) (a = 0: p itself, bit for bit) is shaded once by vk_light.hpp.
//
// Why skipping stays exact.  Every f32 lerp of the filter stays within its operands (vk_tf.hpp, top), so a sample of a cell lies in
// [m, M], its smallest and largest taps.  A cell with finite taps and M < iso_k therefore holds no sample with x >= iso_k: a skipped step
// and a sampled one agree, and a ray carries nothing else from one step to the next.  A cell with a non-finite tap is never empty (a
// +inf tap is a hit on its own corner; NaN samples are no hit, but the same cell can hold finite samples above the threshold).
#pragma once

#include <math.h>
#include <stdint.h>

#include "vk_light.hpp"
#include "vk_tf.hpp"  // SampleScale

#if defined(__HIPCC__)
#define VK_ISO_HD __host__ __device__ __forceinline__
#else
#define VK_ISO_HD inline
#endif

namespace vk {

constexpr uint32_t kIsoMaxRefine = 16;   // VK_ISO_MAX_REFINE
constexpr float kIsoMaxColour = 1e30f;   // VK_TF_MAX_COLOUR

// What the isosurface kernels read (a kernel argument of their own).
struct IsoDesc {
    float iso_k;       // the threshold on the kernel's scale
    float r, g, b;     // linear surface colour
    uint32_t refine;   // bisection steps R
    int32_t lit;       // != 0: shade with `light`
    LightDesc light;
};
static_assert(sizeof(IsoDesc) == 56, "IsoDesc: six words and a LightDesc");

// The threshold on the kernel's scale, rounded once to f32: R8 volumes filter their taps on 0..255, R16_UNORM volumes on 0..65535, R16F
// volumes their values.
VK_ISO_HD float iso_k(float iso, SampleScale s) { return s == SCALE_R8 ? iso * 255.0f : (s == SCALE_U16 ? iso * 65535.0f : iso); }
VK_ISO_HD float iso_k(float iso, bool r8) { return iso_k(iso, r8 ? SCALE_R8 : SCALE_VALUE); }

// The hit test: one compare; a NaN sample is no hit, +inf is one.
VK_ISO_HD bool iso_hit(float x, float k) { return x >= k; }

// Emptiness of a cell (f32 taps on the kernel's scale): its 8 taps are finite and the largest lies below the threshold.
VK_ISO_HD bool iso_cell_empty(const float t[8], float k) {
    float M = t[0];
    bool finite = true;
    for (int b = 0; b < 8; b++) {
        finite = finite && isfinite(t[b]);
        M = fmaxf(M, t[b]);
    }
    return finite && M < k;
}

// Host validation of the public parameters (vk_isosurface's fields); fills the descriptor but for its lighting and returns nullptr,
// or returns what is wrong.
inline const char *iso_desc(float iso, const float rgb[3], uint32_t refine, SampleScale s, IsoDesc &D) {
    if (!isfinite(iso)) return "iso is not finite";
    for (int c = 0; c < 3; c++)
        if (!(fabsf(rgb[c]) <= kIsoMaxColour)) return "a colour is not finite or beyond +-VK_TF_MAX_COLOUR";
    if (refine > kIsoMaxRefine) return "refine is above VK_ISO_MAX_REFINE";
    D.iso_k = iso_k(iso, s);
    D.r = rgb[0]; D.g = rgb[1]; D.b = rgb[2];
    D.refine = refine;
    return nullptr;
}
inline const char *iso_desc(float iso, const float rgb[3], uint32_t refine, bool r8, IsoDesc &D) { return iso_desc(iso, rgb, refine, r8 ? SCALE_R8 : SCALE_VALUE, D); }

// One component of a refinement position: m steps back from the hit sample.
VK_ISO_HD float iso_back(float m, float s, float p) { return fmaf(-m, s, p); }

// The bisection: `hits(m)` says whether the sample m steps before the hit position is at or above the threshold.  Returns a.
template <class Hits>
VK_ISO_HD float iso_refine(uint32_t refine, Hits &&hits) {
    float a = 0.0f, h = 0.5f;
    for (uint32_t i = 0; i < refine; i++) {
        const float m = a + h;  // exact: a has at most i bits, h = 2^-(i+1)
        if (hits(m)) a = m;
        h *= 0.5f;
    }
    return a;
}

}  // namespace vk
