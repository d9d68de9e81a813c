// vk_tf.hpp -- the runtime transfer function of NAIVE_TRILINEAR (vk_set_transfer_function): the table coordinate of a sample and the
// emptiness predicate of a cell under the table, shared by the march kernels, the skip-map rebuild (vk_volume.hip) and the host
// fuzz (tests/tf_fuzz.cpp, plain g++ under ASan / UBSan).
//
// x is the filtered sample on the kernel's own scale (R8: the filtered taps on 0..255; R16_UNORM: on 0..65535; R16F: the value).  With k1, k2 from
// tf_constants():  u = min(max(fma(x, k1, k2), 0), n - 1)  (a NaN sample reads entry 0),  i = min(floor(u), n - 2),  f = u - i,
// c = fma(f, T[i+1] - T[i], T[i]) per channel.
//
// Why skipping stays exact.  Every f32 lerp of the filter, fma(f, b - a, a) with 0 <= f < 1, lies in [min(a, b), max(a, b)]: the
// rounded difference times f stays below |b - a| in magnitude, and rounding to nearest never leaves an interval whose ends are
// representable.  So a sample of a cell lies in [m, M], its smallest and largest taps; fma(x, k1, k2) with k1 > 0 rounds once and
// is monotone, so floor(u(x)) is in [floor(u(m)), floor(u(M))] and the lookup reads entries of [floor(u(m)), floor(u(M)) + 1].
// The predicate checks one guard entry more on each side.  If all of them have alpha 0, c.a = fma(f, +-0 - +-0, +-0) is +0, the
// weight w = (1 - A) * 0 is +0 and the sample adds +0 to every accumulator: a skipped step and a sampled one leave the same bits.
// (This needs finite colours in the lerp: vk_set_transfer_function refuses |r|, |g|, |b| > VK_TF_MAX_COLOUR = 1e30, so the difference of
// two neighbours, and with it fma(+0, c, G) = G, stays finite.)
// A cell with a non-finite tap is never empty.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VK_TF_HD __host__ __device__ __forceinline__
#else
#define VK_TF_HD inline
#endif

namespace vk {

constexpr int kTfMaxEntries = 256;

// What the table kernels read (a kernel argument of their own: the kernels without a table keep their arguments as they are):
// n RGBA f32 entries and the constants below, umax = n - 1, imax = n - 2.
struct TfDesc {
    const float *rgba;
    float k1, k2, umax;
    int32_t imax;
};

// The kernel's scale S of a volume format: a filtered sample is S times the shader-side value.  R16F: the value itself; R8_UNORM: the
// taps 0..255; R16_UNORM: the taps 0..65535 (every u16 is exact in f32).  The numbers are transfer_alpha<>'s SCALE (vk_common.hpp).
enum SampleScale : int { SCALE_VALUE = 0, SCALE_R8 = 1, SCALE_U16 = 3 };
inline double sample_scale(SampleScale s) { return s == SCALE_R8 ? 255.0 : (s == SCALE_U16 ? 65535.0 : 1.0); }

// k1 = (n-1) / ((hi-lo) S), k2 = -lo (n-1) / (hi-lo), each computed in double and rounded once to f32; S = 255 for R8 volumes, 65535 for R16_UNORM, 1 for R16F
inline void tf_constants(uint32_t n, float lo, float hi, SampleScale s, float &k1, float &k2) {
    const double span = (double)hi - (double)lo, nm1 = (double)n - 1.0;
    k1 = (float)(nm1 / (span * sample_scale(s)));
    k2 = (float)(-(double)lo * nm1 / span);
}
inline void tf_constants(uint32_t n, float lo, float hi, bool r8, float &k1, float &k2) { tf_constants(n, lo, hi, r8 ? SCALE_R8 : SCALE_VALUE, k1, k2); }

// the table coordinate u in [0, n - 1] (umax = n - 1)
VK_TF_HD float tf_u(float x, float k1, float k2, float umax) { return fminf(fmaxf(fmaf(x, k1, k2), 0.0f), umax); }

// the lower entry of the lerp (imax = n - 2)
VK_TF_HD int tf_index(float u, int imax) {
    const int i = (int)floorf(u);
    return i < imax ? i : imax;
}

// prefix[j] = number of entries among T[0 .. j-1] whose alpha is not 0 (n + 1 values): the predicate is O(1) per cell
inline void tf_alpha_prefix(const float *rgba, uint32_t n, uint32_t *prefix) {
    prefix[0] = 0;
    for (uint32_t j = 0; j < n; j++) prefix[j + 1] = prefix[j] + (rgba[4 * j + 3] != 0.0f ? 1u : 0u);
}

// Emptiness of a cell with finite taps in [m, M]: every entry of [max(floor(u(m)) - 1, 0), min(floor(u(M)) + 2, n - 1)] has alpha 0.
VK_TF_HD bool tf_range_empty(float m, float M, const uint32_t *prefix, int n, float k1, float k2) {
    const float umax = (float)(n - 1);
    int lo = (int)floorf(tf_u(m, k1, k2, umax)) - 1, hi = (int)floorf(tf_u(M, k1, k2, umax)) + 2;
    lo = lo < 0 ? 0 : lo;
    hi = hi > n - 1 ? n - 1 : hi;
    return prefix[hi + 1] == prefix[lo];
}

// The same for a cell's eight taps (f32 values on the kernel's scale); false as soon as one tap is not finite.
VK_TF_HD bool tf_cell_empty(const float t[8], const uint32_t *prefix, int n, float k1, float k2) {
    float m = t[0], M = t[0];
    bool finite = true;
    for (int b = 0; b < 8; b++) {
        finite = finite && isfinite(t[b]);
        m = fminf(m, t[b]);
        M = fmaxf(M, t[b]);
    }
    return finite && tf_range_empty(m, M, prefix, n, k1, k2);
}

// The emptiness predicate of the built-in transfer (no table): a tap is empty when transfer_alpha gives +0 for every sample that lerps it
// with other empty taps.  u8 (the tap's value 0..255): t <= 25, since 25/255 < 0.1 <= 26/255.  f16: t finite and t <= 0.1f.  A NaN or an
// infinite tap is never empty: the filter's fma(f, b - a, a) turns an infinite tap into NaN (inf - inf, 0 * inf) and
// transfer_alpha(NaN) = smoothstep of min(NaN, 0.9) = 0.9, alpha ~0.817 -- the same for -inf as for +inf.  Shared by pack_cells_kernel,
// cell_occ_kernel's built-in branch and the host fuzz (tests/builtin_fuzz.cpp); the oracle and the numpy restatement state it again.
// u16 (the tap's value 0..65535): t <= 6553.  transfer_alpha<3> computes s = fma(min(t, 58981.5), k1, k2), k1 = f32(1 / (65535 * 1.1)),
// k2 = f32(-0.1 / 1.1): fma(6553, k1, k2) = -6.94e-6, clamped to +0, and fma(6554, k1, k2) = +6.93e-6 (tests/u16_fuzz.cpp walks all 65536
// values).  A sample that lerps taps <= 6553 stays <= 6553 (the argument at the top of this file) and the fma is monotone: its alpha is +0.
VK_TF_HD bool builtin_tap_empty(float t, SampleScale s) {
    return s == SCALE_VALUE ? (isfinite(t) && t <= 0.1f) : (s == SCALE_U16 ? t <= 6553.0f : t <= 25.0f);
}
VK_TF_HD bool builtin_tap_empty(float t, bool f16) { return builtin_tap_empty(t, f16 ? SCALE_VALUE : SCALE_R8); }

// The same for a cell's eight taps (f32 values: u8 taps on 0..255, u16 taps on 0..65535, f16 taps as values): empty when every tap is.
VK_TF_HD bool builtin_cell_empty(const float t[8], SampleScale s) {
    bool empty = true;
    for (int b = 0; b < 8; b++) empty = empty && builtin_tap_empty(t[b], s);
    return empty;
}
VK_TF_HD bool builtin_cell_empty(const float t[8], bool f16) { return builtin_cell_empty(t, f16 ? SCALE_VALUE : SCALE_R8); }

// ---- lone-speckle cells of the built-in transfer (u8 cells: P8 and P16) ----
// A cell with exactly one tap above the threshold (v > 25 at corner dx | dy << 1 | dz << 2, every other tap <= m <= 25) is not empty,
// yet most samples inside it filter to a value that transfer_alpha<1> clamps to +0.  Its distance byte says how close a sample may
// come to the hot corner for that to be certain:
//   speckle_code:    0x80 | corner << 4 | q,  q = floor(16 (25 - m) / (v - m)) in 1 .. 15  (v > 25 >= m: the quotient is below 16);
//                    0 for any other cell -- no tap or several taps above 25, q = 0, a tap that is no u8 value.  For u8 taps the f32
//                    division is exact: numerator and denominator are integers <= 400, and a quotient that is no integer is at
//                    least 1/255 away from one.  f16 cells are never coded, so no tap here is NaN or infinite.  A border cell's
//                    clamped taps repeat a hot voxel: two or more hot taps, not coded.
//   speckle_proven:  w < q / 16, w = (wx wy) wz the trilinear weight of the hot corner, w_i = f_i toward the corner's upper side and
//                    1 - f_i toward its lower side -- written |f_i - o_i| with o_i = 1 - (corner bit i), which is the same f32 value
//                    (a subtraction, its sign dropped) and needs no select.
// Proof that a proven sample's alpha is +0, with the margin.  In exact arithmetic the filter is sum_i w_i t_i over the eight corners,
// the weights >= 0 with sum 1, so it is at most w v + (1 - w) m = m + w (v - m).
//   (a) the decoder's w.  1 - f rounds once (<= 2^-25 absolute; f, and with it every w_i, is in [0, 1]), each product once (2^-24
//       relative): the exact weight is below the computed one plus 2^-22.  q / 16 is exact.  So computed w < q / 16 gives an exact
//       filter value below m + (q / 16)(v - m) + 255 * 2^-22 <= 25 + 6.1e-5, by the definition of q.
//   (b) the f32 chain, for both layouts: x-lerps fma(fx, t1 - t0, t0) on exact differences (P8: of integers; P16: the stored f16
//       delta, exact for u8 data -- xlerp_cell), then c0 = fma(fy, c10 - c00, c00), c1 likewise, r = fma(fz, c1 - c0, c0).  Every
//       intermediate lies between its operands (the argument at the top of this file), so in [0, 255], where one rounding is at most
//       2^-17.  An x-lerp is off by <= 2^-17; each later level adds the rounding of its difference and its own: <= 3 * 2^-17 after y,
//       <= 5 * 2^-17 = 3.9e-5 after z.
//   (c) so r < 25 + 1.1e-4.  transfer_alpha<1> computes s = fma(min(r, 229.5), k1, k2) with k1 = f32(1 / 280.5), k2 = f32(-1 / 11):
//       s <= 0 exactly when r k1 <= -k2 up to one rounding, i.e. for every r <= 25.4 (25.4 k1 = 0.09055 against 0.09091: a relative gap
//       of 4e-3, thousands of roundings wide); fmaxf(s, 0) is then +0 and alpha = (0 * 0) * 3 = +0.  The margin between what (a)
//       and (b) allow, 25.0001, and what (c) needs, 25.4, is why q carries no margin of its own.
// A NaN weight (the position of a ray that left the finite range) compares false: not proven, the sample is evaluated as before.
VK_TF_HD uint32_t speckle_code(const float t[8]) {
    int hot = 0, n_hot = 0;
    float m = 0.0f;
    for (int b = 0; b < 8; b++) {
        if (!(t[b] >= 0.0f && t[b] <= 255.0f)) return 0;
        if (t[b] > 25.0f) { hot = b; n_hot++; }
        else m = fmaxf(m, t[b]);
    }
    if (n_hot != 1) return 0;
    const float q = floorf(16.0f * (25.0f - m) / (t[hot] - m));
    if (!(q >= 1.0f)) return 0;
    return 0x80u | ((uint32_t)hot << 4) | (uint32_t)q;
}

// the decoder with the corner's o_i in hand (the march keeps the eight corners' in LDS, kSpeckleLutBytes: one read instead of the bit work)
VK_TF_HD bool speckle_below(uint32_t code, float ox, float oy, float oz, float fx, float fy, float fz) {
    return (fabsf(fx - ox) * fabsf(fy - oy)) * fabsf(fz - oz) < (float)(code & 15u) * 0.0625f;
}
VK_TF_HD bool speckle_proven(uint32_t code, float fx, float fy, float fz) {
    const uint32_t lower = ~code;  // bit 4 + i set: the hot corner is on the lower side of axis i, its weight there 1 - f
    return speckle_below(code, (float)((lower >> 4) & 1u), (float)((lower >> 5) & 1u), (float)((lower >> 6) & 1u), fx, fy, fz);
}

// ---- maximum-intensity projection (vk_set_projection(VK_PROJ_MAX)) ----
// One step of the running maximum in table coordinates: U' = fmaxf(U, tf_u(x)) with the rule that a U comparing equal to zero is +0.
// Written as a select: with 0 <= U <= umax (U starts at +0), u = fma(x, k1, k2) replaces U only when u > U, which is never the case
// for u <= 0, u = -0 or a NaN u (a NaN sample reads as the minimum); the result is clamped to umax.  For u > U >= 0 that is
// min(max(u, 0), umax) = tf_u(x), otherwise U: the specification's value, and U never carries a -0.
VK_TF_HD float mip_update(float U, float x, float k1, float k2, float umax) {
    const float u = fmaf(x, k1, k2);
    return fminf(u > U ? u : U, umax);
}

// Emptiness of a cell under the maximum projection: its 8 taps are finite and tf_u(M) == 0 for its largest tap M.  Why skipping stays
// exact: a sample of the cell lies in [m, M] (the lerp argument at the top of this file), fma(x, k1, k2) with k1 > 0 rounds once and
// is monotone in x, so u(x) <= u(M) <= 0 and mip_update leaves U with the bits it had -- a skipped step and a sampled one agree.
// A cell with a non-finite tap is never empty (its samples can be NaN or +inf).
VK_TF_HD bool mip_cell_empty(const float t[8], float k1, float k2, float umax) {
    float M = t[0];
    bool finite = true;
    for (int b = 0; b < 8; b++) {
        finite = finite && isfinite(t[b]);
        M = fmaxf(M, t[b]);
    }
    return finite && tf_u(M, k1, k2, umax) == 0.0f;
}

}  // namespace vk
