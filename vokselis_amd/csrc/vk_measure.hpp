// vk_measure.hpp -- measure labelled regions (vk_measure_components): the validation of a caller's
// vk_measure_request, the integer scale q of a stored texel, the limbs in which q and q q are summed and their join, the closed forms of a
// run's index sums, the overflow test of those sums and the layout of a region's record on the device, for the kernels and their host
// (vk_launch_measure.hip); plain C++ that g++ compiles without a device, as vk_label.hpp and vk_split.hpp are, so that a host fuzz can
// share it (tests/measure_fuzz.cpp).  The label array's chunk arithmetic is the label pass's (vk_label.hpp).
#pragma once

#include "vk_label.hpp"

namespace vk {

// ---- the request -------------------------------------------------------------------------------------------------------------
// A caller's request without the volume (the box against the volume, max_label against the voxel count, the volume's kind and the
// overflow bound are the entry point's).  Returns nullptr, or what is wrong (VK_ERR_INVALID).
inline const char *measure_validate(const vk_measure_request *r, bool have_labels_in, bool have_box, bool have_regions, uint64_t cap_regions, bool have_result) {
    if (!r) return "the request is NULL";
    if (isnan(r->lo) || isnan(r->hi)) return "lo or hi is NaN";
    if (r->lo > r->hi) return "lo > hi";
    if (!have_labels_in && r->connectivity != 6u && r->connectivity != 18u && r->connectivity != 26u) return "connectivity must be 6, 18 or 26";
    if (r->flags & ~(uint32_t)VK_MEASURE_CLIP_BOX) return "unknown flag (VK_MEASURE_CLIP_BOX)";
    if (r->pad != 0u) return "pad must be 0";
    if (have_regions && cap_regions == 0u) return "regions with cap_regions == 0";
    if (!have_regions && !have_result) return "neither regions nor result: the result would go nowhere";
    if (have_labels_in) {
        if (r->lo != 0.0f || r->hi != 0.0f || r->connectivity != 0u) return "lo, hi and connectivity must be 0 with labels_in: the labels say what a region is";
        if (have_box || (r->flags & VK_MEASURE_CLIP_BOX)) return "a box or VK_MEASURE_CLIP_BOX with labels_in: the labels cover the whole volume";
        if (r->max_label == 0u) return "max_label == 0 with labels_in";
    } else if (r->max_label != 0u) return "max_label != 0 without labels_in";
    return nullptr;
}

// Whether no index sum of a region can overflow 64 bits: the largest is below n (m - 1)^2, n the voxels and m the largest dimension
// (VK_ERR_UNSUPPORTED otherwise).  m - 1 < 2^32, so its square fits.
inline bool measure_sums_fit(uint32_t nx, uint32_t ny, uint32_t nz) {
    const uint64_t n = (uint64_t)nx * ny * nz, m = std::max(nx, std::max(ny, nz));
    const uint64_t sq = (m - 1u) * (m - 1u);
    return n == 0u || sq == 0u || n <= UINT64_MAX / sq;
}

// ---- q: the stored texel on an integer scale ---------------------------------------------------------------------------------
constexpr uint32_t kMeasureScaleF16 = 1u << 24;
// the divisor from q to the sample value; format: VK_FMT_*
inline uint32_t measure_scale(int format) { return format == VK_FMT_R8_UNORM ? 255u : (format == VK_FMT_R16_UNORM ? 65535u : kMeasureScaleF16); }
// A half's bits h as t 2^24: a subnormal m 2^-24 is m, a normal (1024 + m) 2^(e - 25) is (1024 + m) 2^(e - 1) < 2^40; -0 is 0.
// finite: false for NaN and +-inf (q is 0 then).
VK_LABEL_HD int64_t measure_q_half(uint32_t h, bool &finite) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    finite = e != 31u;
    if (!finite) return 0;
    const int64_t a = e == 0u ? (int64_t)m : (int64_t)(m | 1024u) << (e - 1u);
    return (h & 0x8000u) ? -a : a;
}

// ---- limbs ---------------------------------------------------------------------------------------------------------------------
// A region has at most 2^32 - 2 voxels, so a limb below 2^31 in magnitude sums into 64 bits.  q = hi 2^20 + lo with lo its low 20 bits and
// hi the arithmetic high part (|hi| <= 2^20); q q < 2^80 in three limbs of 28 bits.  The integer formats put q (< 2^16) and q q (< 2^32)
// whole into the lowest limb and leave the others 0: the join is the same.
constexpr uint32_t kMeasureQShift = 20, kMeasureQQShift = 28;
VK_LABEL_HD void measure_q_split(int64_t q, int64_t &hi, uint64_t &lo) {
    lo = (uint64_t)q & ((1ull << kMeasureQShift) - 1u);
    hi = q >> kMeasureQShift;  // arithmetic
}
VK_LABEL_HD void measure_qq_split(int64_t q, uint64_t limb[3]) {
    const uint64_t a = (uint64_t)(q < 0 ? -q : q);                     // < 2^40
    const uint64_t ah = a >> 20, al = a & 0xfffffu;                    // a = ah 2^20 + al, both < 2^20
    // a a = ah ah 2^40 + 2 ah al 2^20 + al al; every product is below 2^40, so each line below stays inside 64 bits
    const uint64_t mask = (1ull << kMeasureQQShift) - 1u;
    const uint64_t mid = 2u * ah * al;                                 // < 2^41, weight 2^20
    uint64_t t = al * al + ((mid & 0xffu) << 20);                      // weight 1: < 2^40 + 2^28
    limb[0] = t & mask;
    t = (t >> kMeasureQQShift) + (mid >> 8) + ((ah * ah & 0xffffu) << 12);  // weight 2^28: mid's bits from 8 up, ah ah's low 16 bits at 2^(40 - 28)
    limb[1] = t & mask;
    limb[2] = (t >> kMeasureQQShift) + (ah * ah >> 16);                // weight 2^56
}
#if defined(__SIZEOF_INT128__)
// the joins (host): the limbs' sums as the record's 128-bit fields
inline void measure_q_join(int64_t sum_hi, uint64_t sum_lo, int64_t &out_hi, uint64_t &out_lo) {
    const __int128 s = (__int128)sum_hi * ((__int128)1 << kMeasureQShift) + (__int128)sum_lo;
    out_lo = (uint64_t)s;
    out_hi = (int64_t)(s >> 64);
}
inline void measure_qq_join(const uint64_t sum[3], uint64_t &out_hi, uint64_t &out_lo) {
    const unsigned __int128 s = (unsigned __int128)sum[0] + ((unsigned __int128)sum[1] << kMeasureQQShift) + ((unsigned __int128)sum[2] << (2u * kMeasureQQShift));
    out_lo = (uint64_t)s;
    out_hi = (uint64_t)(s >> 64);
}
#endif

// ---- a run ---------------------------------------------------------------------------------------------------------------------
// The nine index sums of the voxels (x, y, z), (x + 1, y, z), ..., (x + len - 1, y, z): s = x, y, z, xx, yy, zz, xy, xz, yz.
VK_LABEL_HD void measure_run_sums(uint64_t x, uint64_t y, uint64_t z, uint64_t len, uint64_t s[9]) {
    const uint64_t tri = len * (len - 1u) / 2u;                        // 0 + 1 + ... + (len - 1)
    const uint64_t sq = (len - 1u) * len * (2u * len - 1u) / 6u;       // 0 + 1 + 4 + ... + (len - 1)^2
    s[0] = len * x + tri;
    s[1] = len * y;
    s[2] = len * z;
    s[3] = len * x * x + 2u * x * tri + sq;
    s[4] = len * y * y;
    s[5] = len * z * z;
    s[6] = y * s[0];
    s[7] = z * s[0];
    s[8] = len * y * z;
}

// ---- a region's record on the device -----------------------------------------------------------------------------------------
// kMeasureWords words of 64 bits per region, each gathered by one kind of integer atomic (add, unsigned min / max, signed min / max), so
// the order of the atomics does not show.  The words an integer format never touches come last: its kernels keep a shorter table.
enum MeasureWord : uint32_t {
    MW_N = 0, MW_FIRST = 1, MW_BOX_LO = 2, MW_BOX_HI = 5, MW_SUMS = 8, MW_FACES = 17, MW_QMIN = 20, MW_QMAX = 21, MW_Q_LO = 22, MW_QQ0 = 23,
    MW_NONFINITE = 24, MW_Q_HI = 25, MW_QQ1 = 26, MW_QQ2 = 27
};
constexpr uint32_t kMeasureWords = 28, kMeasureWordsInt = 24;
enum MeasureOp : uint32_t { MOP_ADD, MOP_UMIN, MOP_UMAX, MOP_SMIN, MOP_SMAX };
VK_LABEL_HD MeasureOp measure_word_op(uint32_t k) {
    return (k >= MW_FIRST && k < MW_BOX_HI) ? MOP_UMIN : ((k >= MW_BOX_HI && k < MW_SUMS) ? MOP_UMAX : (k == MW_QMIN ? MOP_SMIN : (k == MW_QMAX ? MOP_SMAX : MOP_ADD)));
}
// what a word holds before anything was gathered: the operation's neutral element
VK_LABEL_HD uint64_t measure_word_init(uint32_t k) {
    const MeasureOp op = measure_word_op(k);
    return op == MOP_UMIN ? UINT64_MAX : (op == MOP_SMIN ? (uint64_t)INT64_MAX : (op == MOP_SMAX ? (uint64_t)INT64_MIN : 0u));
}
#if defined(__SIZEOF_INT128__)
// a device record as the caller's (host)
inline vk_region measure_region(const uint64_t *w) {
    vk_region r{};
    r.n_voxels = w[MW_N];
    r.first = w[MW_FIRST];
    if (r.n_voxels)
        r.box = vk_voxel_box{(uint32_t)w[MW_BOX_LO], (uint32_t)w[MW_BOX_LO + 1], (uint32_t)w[MW_BOX_LO + 2], (uint32_t)w[MW_BOX_HI] + 1u, (uint32_t)w[MW_BOX_HI + 1] + 1u, (uint32_t)w[MW_BOX_HI + 2] + 1u};
    r.sum_x = w[MW_SUMS]; r.sum_y = w[MW_SUMS + 1]; r.sum_z = w[MW_SUMS + 2];
    r.sum_xx = w[MW_SUMS + 3]; r.sum_yy = w[MW_SUMS + 4]; r.sum_zz = w[MW_SUMS + 5];
    r.sum_xy = w[MW_SUMS + 6]; r.sum_xz = w[MW_SUMS + 7]; r.sum_yz = w[MW_SUMS + 8];
    r.n_nonfinite = w[MW_NONFINITE];
    r.q_min = (int64_t)w[MW_QMIN];
    r.q_max = (int64_t)w[MW_QMAX];
    measure_q_join((int64_t)w[MW_Q_HI], w[MW_Q_LO], r.sum_q_hi, r.sum_q_lo);
    const uint64_t qq[3] = {w[MW_QQ0], w[MW_QQ1], w[MW_QQ2]};
    measure_qq_join(qq, r.sum_qq_hi, r.sum_qq_lo);
    for (int a = 0; a < 3; a++) r.faces[a] = w[MW_FACES + a];
    return r;
}
#endif

// the workgroup's table: slots found by the top bits of label_slot's hash, no probing
constexpr uint32_t kMeasureSlotBits = 7, kMeasureSlots = 1u << kMeasureSlotBits;
VK_LABEL_HD uint32_t measure_slot(uint32_t id) { return (id * 2654435761u) >> (32u - kMeasureSlotBits); }

}  // namespace vk
