// vk_pair.hpp -- the emptiness predicate of the compute twin's 16-byte records (COMPUTE_NEAREST, raycast_compute.wgsl:62-97), shared by
// pack_pairs_kernel (vk_volume_kernels.hpp: the seed of the records' skip map) and the host fuzz (tests/compute_fuzz.cpp, plain g++ under
// ASan / UBSan).
//
// A record may be walked over -- not fetched, not shaded -- only if shading it would leave every accumulator as it is.  Its step adds
// w * col * shade to each colour channel and w to A, with w = (1 - A) * smoothstep(0, 0.7, a^3).  When that smoothstep is exactly 0
// (a <= 0, a NaN, or an a^3 so small that s * s underflows), w is +0 and the step adds w * col * shade = +-0 -- but only while col and
// shade are finite: +0 times an infinity is NaN.  In the records kernel's form of the step (vk_compute.hpp),
//   col_k = rgb_k + 3 c_k dl ss   with dl = max(dot(n, l1), 0), l1 = normalize(-2, -2, -1), ss in [0, 1],
//   shade = max(0, -n.y) (* 0.8, + a finite blue term),
// so col is finite iff rgb is finite and dl is; dl is infinite only if dot(n, l1) = +inf, which needs a -inf component (every l1 component
// is negative and f16 magnitudes cannot overflow the sum); shade is infinite iff n.y = -inf.  A record is therefore empty iff its opacity
// term is 0, its three colour halves are finite and no normal component is -inf.  +inf components and NaNs are harmless: max() drops a
// NaN, and +inf times a negative l1 component or negated is -inf, which max(., 0) turns into 0.  So the xor example's holes (zero
// opacity, NaN normals) stay empty.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VK_PAIR_HD __host__ __device__ __forceinline__
#else
#define VK_PAIR_HD inline
#endif

namespace vk {

// raycast_compute.wgsl:78-79: smoothstep(0.0, 0.7, pow(a, 3.0)), specified as a * a * a and smoothstep's reciprocal form -- the same
// operations as vk_common.hpp's smoothstepf(0, 0.7, .) in the march kernels
VK_PAIR_HD float pair_opacity(float a) {
    const float inv = 1.0f / (0.7f - 0.0f);
    float s = ((a * a) * a - 0.0f) * inv;
    s = fminf(fmaxf(s, 0.0f), 1.0f);
    return (s * s) * fmaf(-2.0f, s, 3.0f);
}

// rgba: the record's density half (colour, opacity), n: its normal half (x, y, z), each an f16 widened exactly to f32
VK_PAIR_HD bool pair_record_empty(const float rgba[4], const float n[3]) {
    return pair_opacity(rgba[3]) == 0.0f && isfinite(rgba[0]) && isfinite(rgba[1]) && isfinite(rgba[2]) && n[0] != -INFINITY &&
           n[1] != -INFINITY && n[2] != -INFINITY;
}

}  // namespace vk
