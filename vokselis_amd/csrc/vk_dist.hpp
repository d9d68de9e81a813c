// vk_dist.hpp -- exact Euclidean distance transform of a value range and morphology by a radius (vk_distance_transform; DESIGN.md
// section 25): the validation of a caller's vk_distance_request, the overflow bound, R2, what each op's rounds look for, and the line
// function -- the lower envelope of parabolas along one line, in integers -- shared by the kernels and their host
// (vk_launch_dist.hip) and the host fuzz (tests/dist_fuzz.cpp, plain g++ under ASan / UBSan).
//
// The transform is separable: D2(A, v) = min_z' min_y' min_x' [...] and the three minima nest.  The first pass, along z, finds the squared
// distance to the nearest voxel of A in v's own column.  Each later pass replaces g along a line by
//     out(i) = min over j with g(j) != INF of g(j) + (w (i - j))^2,
// the lower envelope of one parabola per entry, all of the same curvature w^2: dist_line.  The result does not depend on the axis order.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vokselis_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VK_DIST_HD __host__ __device__ __forceinline__
#else
#define VK_DIST_HD inline
#endif

namespace vk {

constexpr uint32_t kDistInf = VK_DIST_INF;
constexpr uint64_t kDistMaxVoxels = 0xfffffffeull;  // as the label pass: voxel indices are 32-bit
constexpr uint64_t kDistMaxD2 = 0xfffffffeull;      // the largest finite D2

// ---- the request -------------------------------------------------------------------------------------------------------------
inline bool dist_is_morph(int32_t op) { return op >= VK_DIST_DILATE && op <= VK_DIST_OPEN; }
// A caller's request without the volume (the box, the volume's kind and the overflow bound are the entry point's).  Returns nullptr,
// or what is wrong (VK_ERR_INVALID).
inline const char *dist_validate(const vk_distance_request *r, bool have_d2, bool have_dense, bool have_result) {
    if (!r) return "the request is NULL";
    if (isnan(r->lo) || isnan(r->hi)) return "lo or hi is NaN";
    if (r->lo > r->hi) return "lo > hi";
    if (r->op < VK_DIST_OUTSIDE || r->op > VK_DIST_OPEN) return "unknown op (VK_DIST_OUTSIDE, _INSIDE, _DILATE, _ERODE, _CLOSE, _OPEN)";
    if (r->flags & ~(uint32_t)(VK_DIST_CLIP_BOX | VK_DIST_INSTALL)) return "unknown flag (VK_DIST_CLIP_BOX, VK_DIST_INSTALL)";
    for (int c = 0; c < 3; c++)
        if (r->spacing[c] < 1u || r->spacing[c] > (uint32_t)VK_DIST_MAX_SPACING) return "a spacing outside 1 .. VK_DIST_MAX_SPACING";
    if (!isfinite(r->radius) || r->radius < 0.0f || r->radius > VK_DIST_MAX_RADIUS) return "the radius is not finite, is negative or lies above VK_DIST_MAX_RADIUS";
    if (!isfinite(r->fill_in) || !isfinite(r->fill_out)) return "a fill is not finite";
    const bool install = (r->flags & VK_DIST_INSTALL) != 0u;
    if (dist_is_morph(r->op)) {
        if (have_d2) return "d2_out with a morphology op (VK_DIST_OUTSIDE and VK_DIST_INSIDE write it)";
        if (!have_dense && !install && !have_result) return "none of dense_out, VK_DIST_INSTALL and result: the result would go nowhere";
    } else {
        if (r->radius != 0.0f) return "a radius with a distance op (it must be 0)";
        if (have_dense || install) return "dense_out or VK_DIST_INSTALL with a distance op (the morphology ops write a volume)";
        if (!have_d2 && !have_result) return "neither d2_out nor result: the result would go nowhere";
    }
    return nullptr;
}
// sum_c (spacing[c] (n_c - 1))^2 <= 0xFFFFFFFE: every finite D2 fits (VK_ERR_UNSUPPORTED otherwise).  *bound: the sum, where it fits.
inline bool dist_d2_fits(const uint32_t spacing[3], uint32_t nx, uint32_t ny, uint32_t nz, uint64_t *bound = nullptr) {
    const uint32_t n[3] = {nx, ny, nz};
    uint64_t sum = 0;
    for (int c = 0; c < 3; c++) {
        const uint64_t a = (uint64_t)spacing[c] * (uint64_t)(n[c] ? n[c] - 1u : 0u);  // < 2^38
        if (a > 0xffffull) return false;                                                // a^2 >= 2^32 on its own
        sum += a * a;
    }
    if (bound) *bound = sum;
    return sum <= kDistMaxD2;
}
inline uint64_t dist_r2(float radius) { return (uint64_t)floor((double)radius * (double)radius); }

// What a round of the three passes measures the distance to, and what the result is compared with.  A round's target is either S or
// not S (the first round), or the voxels whose first-round D2 lies above R2 (the second round of CLOSE and OPEN):
//     CLOSE  M1 = dil(S) = { D2(S) <= R2 }; ero(M1) measures to not M1 = { D2(S) > R2 }
//     OPEN   M1 = ero(S) = { D2(not S) > R2 }; dil(M1) measures to M1 itself
// -- the same test either way.  M is then { D2 <= R2 } for DILATE and OPEN and { D2 > R2 } for ERODE and CLOSE.
VK_DIST_HD bool dist_first_target_is_complement(int32_t op) { return op == VK_DIST_INSIDE || op == VK_DIST_ERODE || op == VK_DIST_OPEN; }
VK_DIST_HD bool dist_two_rounds(int32_t op) { return op == VK_DIST_CLOSE || op == VK_DIST_OPEN; }
VK_DIST_HD bool dist_result_is_above(int32_t op) { return op == VK_DIST_ERODE || op == VK_DIST_CLOSE; }
VK_DIST_HD bool dist_in_result(uint32_t d2, uint64_t r2, bool above) { return ((uint64_t)d2 > r2) == above; }

// ---- the column pass ---------------------------------------------------------------------------------------------------------
// Steps to the nearest target along a column as a squared distance: (w steps)^2, or INF.  w steps <= 0xffff under dist_d2_fits.
VK_DIST_HD uint32_t dist_step_advance(uint32_t steps, bool target) { return target ? 0u : (steps == kDistInf ? kDistInf : steps + 1u); }
VK_DIST_HD uint32_t dist_steps_squared(uint32_t steps, uint32_t w) {
    if (steps == kDistInf) return kDistInf;
    const uint32_t a = w * steps;
    return a * a;
}

// ---- the line function -------------------------------------------------------------------------------------------------------
// A line's stack entry: the parabola's site s (low half) and the first index t it governs (high half).  Both are < 2^16: a line has at
// most 65536 entries under dist_d2_fits.
constexpr uint32_t kDistMaxLine = 65536;
VK_DIST_HD uint32_t dist_entry(uint32_t s, uint32_t t) { return s | (t << 16); }
// the parabola of site j, of height gj, at index x
VK_DIST_HD uint64_t dist_parabola(uint32_t gj, uint32_t j, uint32_t x, uint32_t w) {
    const uint64_t a = (uint64_t)w * (uint64_t)(x > j ? x - j : j - x);
    return (uint64_t)gj + a * a;
}
// Sep: the last index at which the parabola of site i (height gi) is not above that of site u > i (height gu):
// floor((w^2 (u^2 - i^2) + gu - gi) / (2 w^2 (u - i))), in integers.  The numerator stays below 2^33 in magnitude, the divisor below 2^24.
VK_DIST_HD int64_t dist_sep(uint32_t i, uint32_t gi, uint32_t u, uint32_t gu, uint32_t w) {
    const int64_t w2 = (int64_t)w * (int64_t)w;
    const int64_t num = w2 * ((int64_t)u * u - (int64_t)i * i) + (int64_t)gu - (int64_t)gi;
    const uint32_t den = (uint32_t)(2 * w2) * (u - i);
    if (num < 0) return -(int64_t)(((uint64_t)(-num) + den - 1u) / den);   // floor, not truncation (does not occur after the pops: kept exact anyway)
    if (((uint64_t)num >> 32) == 0u) return (int64_t)((uint32_t)num / den);  // the common case in 32 bits
    return (int64_t)((uint64_t)num / den);
}

// out(i) = min over j with g(j) != INF of g(j) + (w (i - j))^2 for i = 0 .. n - 1, INF everywhere when no such j exists.  Entry k of
// g, stack and out sits at [base + k stride]; g and out must not overlap (a site may lie outside the stretch it governs); stack holds n
// entries.  1 <= n <= kDistMaxLine, and every finite result must fit below INF (dist_d2_fits).  Meijster's two scans:
//   build      u walks 0 .. n - 1.  A trip either pops the stack's top -- its parabola lies above u's where it begins, so it governs
//              nothing -- or is done with u: skips it (INF: no parabola), or pushes it at most once.  Pops <= pushes <= n and n trips
//              advance u: at most 2 n trips.  The top's site, start and height stay in registers.
//   read-back  i walks n - 1 .. 0 and evaluates the parabola that governs it: n trips.
// Returns the trips of both scans (the fuzz holds them to 2 n and n).
struct DistTrips { uint32_t build, read; };
VK_DIST_HD DistTrips dist_line(const uint32_t *g, uint32_t *stack, uint32_t *out, uint64_t base, uint64_t stride, uint32_t n, uint32_t w) {
    int32_t q = -1;  // the stack's top
    uint32_t ts = 0u, tt = 0u, tg = 0u;
    uint32_t trips = 0u, u = 0u;
    uint32_t gu = g[base];
    while (u < n && trips < 2u * n) {
        trips++;
        bool done = true;
        if (gu != kDistInf) {
            if (q < 0) {
                q = 0; ts = u; tt = 0u; tg = gu;
                stack[base] = dist_entry(ts, tt);
            } else if (dist_parabola(tg, ts, tt, w) > dist_parabola(gu, u, tt, w)) {
                q--;
                if (q >= 0) {
                    const uint32_t e = stack[base + (uint64_t)q * stride];
                    ts = e & 0xffffu; tt = e >> 16;
                    tg = g[base + (uint64_t)ts * stride];
                }
                done = false;
            } else {
                const int64_t from = 1 + dist_sep(ts, tg, u, gu, w);
                if (from < (int64_t)n) {
                    q++; ts = u; tt = (uint32_t)from; tg = gu;
                    stack[base + (uint64_t)q * stride] = dist_entry(ts, tt);
                }
            }
        }
        if (done) {
            u++;
            if (u < n) gu = g[base + (uint64_t)u * stride];
        }
    }
    uint32_t reads = 0u;
    for (uint32_t k = n; k-- > 0u;) {
        reads++;
        if (q < 0) { out[base + (uint64_t)k * stride] = kDistInf; continue; }
        out[base + (uint64_t)k * stride] = (uint32_t)dist_parabola(tg, ts, k, w);
        if (k == tt && q > 0) {
            q--;
            const uint32_t e = stack[base + (uint64_t)q * stride];
            ts = e & 0xffffu; tt = e >> 16;
            tg = g[base + (uint64_t)ts * stride];
        }
    }
    return DistTrips{trips, reads};
}

}  // namespace vk
