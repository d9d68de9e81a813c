// measure_fuzz.cpp -- vk_measure.hpp on the host, under ASan + UBSan: the request's validation, the overflow test of the index sums at its
// boundary, q of every half, the limbs of q and q q and their joins against __int128, the closed forms of a run against a loop over its
// voxels, and a region's record gathered word by word as the kernel gathers it.  A stand-alone program:
//     measure_fuzz CASES SEED
// Once: (1) the validation's refusals in their order; (2) measure_sums_fit against n (m - 1)^2 in 128 bits, on random shapes and on both
// sides of the boundary for shapes of one, two and three long axes; (3) all 65536 halves: q against ldexp, the split of q and of q q, and
// n = 2^32 - 2 copies of each by multiplication -- no limb's sum leaves 64 bits and the joins give n q and n q q; the integer formats'
// whole q likewise; (4) the run sums for every (x, len) with x + len <= 130.  Per case: (5) a random volume of random labels and halves;
// every row is cut into runs at the label changes and at random further places (a wave's end), every run is gathered into its region's
// 28 words by the words' own operations -- closed forms for the indices, sums of limbs for the texels -- in a shuffled order, and
// measure_region of the words is compared with sums taken voxel by voxel in __int128.
#include "vk_measure.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

using namespace vk;
typedef __int128 i128;
typedef unsigned __int128 u128;

static uint64_t g_state;
static uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// ---- (1) ------------------------------------------------------------------------------------------------------------------------
static void expect(const char *got, const char *want, int line) {
    if (!want) { CHECK(got == nullptr, "line %d: refused with \"%s\"", line, got); return; }
    CHECK(got != nullptr && std::strstr(got, want) != nullptr, "line %d: wanted \"%s\", got \"%s\"", line, want, got ? got : "(accepted)");
}
static vk_measure_request range_request() {
    vk_measure_request r{};
    r.lo = 0.5f; r.hi = INFINITY; r.connectivity = 6u;
    return r;
}
static void check_validation() {
    vk_measure_request r = range_request();
    expect(measure_validate(nullptr, false, false, true, 4u, true), "the request is NULL", __LINE__);
    expect(measure_validate(&r, false, false, true, 4u, true), nullptr, __LINE__);
    expect(measure_validate(&r, false, true, true, 4u, false), nullptr, __LINE__);
    expect(measure_validate(&r, false, false, false, 0u, true), nullptr, __LINE__);
    r.lo = NAN; expect(measure_validate(&r, false, false, true, 4u, true), "NaN", __LINE__);
    r = range_request(); r.hi = NAN; expect(measure_validate(&r, true, false, true, 4u, true), "NaN", __LINE__);
    r = range_request(); r.lo = 0.7f; r.hi = 0.6f; expect(measure_validate(&r, false, false, true, 4u, true), "lo > hi", __LINE__);
    r = range_request(); r.lo = r.hi = 0.5f; expect(measure_validate(&r, false, false, true, 4u, true), nullptr, __LINE__);
    for (uint32_t conn : {0u, 1u, 7u, 19u, 27u, 0xffffffffu}) { r = range_request(); r.connectivity = conn; expect(measure_validate(&r, false, false, true, 4u, true), "connectivity must be 6, 18 or 26", __LINE__); }
    for (uint32_t conn : {6u, 18u, 26u}) { r = range_request(); r.connectivity = conn; expect(measure_validate(&r, false, false, true, 4u, true), nullptr, __LINE__); }
    for (uint32_t flags : {2u, 3u, 0x80000000u}) { r = range_request(); r.flags = flags; expect(measure_validate(&r, false, false, true, 4u, true), "unknown flag", __LINE__); }
    r = range_request(); r.flags = VK_MEASURE_CLIP_BOX; expect(measure_validate(&r, false, false, true, 4u, true), nullptr, __LINE__);
    r = range_request(); r.pad = 1u; expect(measure_validate(&r, false, false, true, 4u, true), "pad must be 0", __LINE__);
    r = range_request(); expect(measure_validate(&r, false, false, true, 0u, true), "cap_regions == 0", __LINE__);
    expect(measure_validate(&r, false, false, false, 0u, false), "the result would go nowhere", __LINE__);
    r.max_label = 1u; expect(measure_validate(&r, false, false, true, 4u, true), "max_label != 0 without labels_in", __LINE__);
    // the order: an earlier refusal wins
    r = range_request(); r.connectivity = 5u; r.flags = 8u; r.pad = 1u; expect(measure_validate(&r, false, false, true, 0u, true), "connectivity", __LINE__);
    r = range_request(); r.flags = 8u; r.pad = 1u; expect(measure_validate(&r, false, false, true, 0u, true), "unknown flag", __LINE__);
    r = range_request(); r.pad = 1u; expect(measure_validate(&r, false, false, true, 0u, true), "pad", __LINE__);
    // with labels_in
    vk_measure_request l{};
    l.max_label = 5u;
    expect(measure_validate(&l, true, false, true, 4u, true), nullptr, __LINE__);
    expect(measure_validate(&l, true, false, false, 0u, true), nullptr, __LINE__);
    expect(measure_validate(&l, true, true, true, 4u, true), "a box or VK_MEASURE_CLIP_BOX with labels_in", __LINE__);
    expect(measure_validate(&l, true, false, true, 0u, true), "cap_regions == 0", __LINE__);
    l.flags = VK_MEASURE_CLIP_BOX; expect(measure_validate(&l, true, false, true, 4u, true), "a box or VK_MEASURE_CLIP_BOX with labels_in", __LINE__);
    l.flags = 0u; l.connectivity = 6u; expect(measure_validate(&l, true, false, true, 4u, true), "must be 0 with labels_in", __LINE__);
    l.connectivity = 0u; l.hi = 1.0f; expect(measure_validate(&l, true, false, true, 4u, true), "must be 0 with labels_in", __LINE__);
    l.hi = 0.0f; l.lo = -0.0f; expect(measure_validate(&l, true, false, true, 4u, true), nullptr, __LINE__);
    l.lo = 0.0f; l.max_label = 0u; expect(measure_validate(&l, true, false, true, 4u, true), "max_label == 0 with labels_in", __LINE__);
    l.max_label = 0xffffffffu; expect(measure_validate(&l, true, false, true, 4u, true), nullptr, __LINE__);  // against the voxel count: the entry point's
}

// ---- (2) ------------------------------------------------------------------------------------------------------------------------
static bool fits_128(uint32_t nx, uint32_t ny, uint32_t nz) {
    const u128 n = (u128)nx * ny * nz, m = std::max(nx, std::max(ny, nz));
    if (m == 0u) return true;
    const u128 once = n * (m - 1u);  // n < 2^96 and m - 1 < 2^32: below 2^128
    return once <= (u128)UINT64_MAX && once * (m - 1u) <= (u128)UINT64_MAX;
}
static void check_overflow_bound() {
    for (int k = 0; k < 200000; k++) {
        const uint32_t s = rnd_below(32u);
        const uint32_t nx = (uint32_t)(rnd() >> (32u + rnd_below(32u))), ny = (uint32_t)(rnd() >> (32u + s)), nz = (uint32_t)(rnd() >> (32u + rnd_below(32u)));
        CHECK(measure_sums_fit(nx, ny, nz) == fits_128(nx, ny, nz), "%u x %u x %u", nx, ny, nz);
    }
    // the boundary along one axis, for one, two and three long axes: the largest m that fits, by bisection on the 128-bit form
    for (int axes = 1; axes <= 3; axes++) {
        auto shape = [&](uint32_t m, uint32_t d[3]) { for (int a = 0; a < 3; a++) d[a] = a < axes ? m : 1u; };
        uint32_t lo = 1u, hi = 0xffffffffu, d[3];
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            shape(mid, d);
            if (fits_128(d[0], d[1], d[2])) lo = mid; else hi = mid;
        }
        shape(lo, d); CHECK(measure_sums_fit(d[0], d[1], d[2]) && fits_128(d[0], d[1], d[2]), "the last shape that fits, %d axes of %u", axes, lo);
        shape(hi, d); CHECK(!measure_sums_fit(d[0], d[1], d[2]) && !fits_128(d[0], d[1], d[2]), "the first shape that does not, %d axes of %u", axes, hi);
        shape(lo, d); CHECK(measure_sums_fit(d[2], d[1], d[0]) && measure_sums_fit(d[1], d[0], d[2]), "the order of the axes");
    }
    CHECK(measure_sums_fit(1024u, 1024u, 1024u) && measure_sums_fit(2048u, 2048u, 1023u) && measure_sums_fit(1u, 1u, 1u) && measure_sums_fit(0u, 5u, 5u), "ordinary volumes");
    CHECK(!measure_sums_fit(1u, 1u, 0xfffffffeu), "a line of 2^32 - 2 voxels");
}

// ---- (3) ------------------------------------------------------------------------------------------------------------------------
static const uint64_t kMostVoxels = kLabelMaxVoxels;  // 2^32 - 2
static void check_limbs_of(int64_t q) {
    int64_t hi; uint64_t lo, limb[3];
    measure_q_split(q, hi, lo);
    CHECK(lo < (1ull << kMeasureQShift) && (i128)hi * (1 << kMeasureQShift) + (i128)lo == (i128)q && hi >= -(1ll << 20) && hi <= (1ll << 20), "q = %lld", (long long)q);
    measure_qq_split(q, limb);
    const u128 qq = (u128)((i128)q * q);
    CHECK(limb[0] < (1ull << 28) && limb[1] < (1ull << 28) && limb[2] < (1ull << 28), "q = %lld: a limb of 28 bits", (long long)q);
    CHECK((u128)limb[0] + ((u128)limb[1] << 28) + ((u128)limb[2] << 56) == qq, "q = %lld: the limbs of q q", (long long)q);
    // 2^32 - 2 copies: every limb's sum stays inside 64 bits, and the joins give the products
    const i128 shi = (i128)hi * kMostVoxels;
    const u128 slo = (u128)lo * kMostVoxels;
    CHECK(shi >= INT64_MIN && shi <= INT64_MAX && slo <= UINT64_MAX, "q = %lld: a limb's sum over 2^32 - 2 voxels", (long long)q);
    int64_t out_hi; uint64_t out_lo;
    measure_q_join((int64_t)shi, (uint64_t)slo, out_hi, out_lo);
    const i128 want = (i128)q * kMostVoxels;
    CHECK(out_lo == (uint64_t)want && out_hi == (int64_t)(want >> 64), "q = %lld: n q", (long long)q);
    uint64_t sums[3], qq_hi, qq_lo;
    for (int m = 0; m < 3; m++) {
        const u128 s = (u128)limb[m] * kMostVoxels;
        CHECK(s <= UINT64_MAX, "q = %lld: limb %d over 2^32 - 2 voxels", (long long)q, m);
        sums[m] = (uint64_t)s;
    }
    measure_qq_join(sums, qq_hi, qq_lo);
    const u128 want2 = qq * kMostVoxels;
    CHECK(qq_lo == (uint64_t)want2 && qq_hi == (uint64_t)(want2 >> 64), "q = %lld: n q q", (long long)q);
}
static void check_q_and_limbs() {
    int64_t most = 0;
    for (uint32_t h = 0; h < 65536u; h++) {
        bool finite;
        const int64_t q = measure_q_half(h, finite);
        const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
        CHECK(finite == (e != 31u), "half %04x", h);
        if (!finite) { CHECK(q == 0, "half %04x", h); continue; }
        double v = e == 0u ? std::ldexp((double)m, -24) : std::ldexp((double)(m + 1024u), (int)e - 25);
        if (h & 0x8000u) v = -v;
        CHECK((double)q == std::ldexp(v, 24) && (q != 0 || (h & 0x7fffu) == 0u), "half %04x: q = %lld", h, (long long)q);
        most = std::max(most, q < 0 ? -q : q);
        check_limbs_of(q);
    }
    CHECK(most == (int64_t)65504 << 24 && most < (1ll << 40), "the largest |q| is 65504 2^24");
    bool finite;
    CHECK(measure_q_half(0x8000u, finite) == 0 && finite && measure_q_half(0x0001u, finite) == 1 && measure_q_half(0x8001u, finite) == -1 && measure_q_half(0x3C00u, finite) == 1 << 24, "-0, the subnormals, 1");
    for (int k = 0; k < 200000; k++) check_limbs_of((int64_t)(rnd() >> 24) - (1ll << 39));  // any q of 40 bits
    check_limbs_of((1ll << 40) - 1); check_limbs_of(-((1ll << 40) - 1)); check_limbs_of(0);
    // the integer formats: q and q q whole in the lowest limb
    for (uint64_t q : {0ull, 1ull, 255ull, 256ull, 65534ull, 65535ull}) {
        const u128 sq = (u128)q * kMostVoxels, sqq = (u128)(q * q) * kMostVoxels;
        CHECK(sq <= UINT64_MAX && sqq <= UINT64_MAX, "q = %llu: the whole sums over 2^32 - 2 voxels", (unsigned long long)q);
        int64_t out_hi; uint64_t out_lo, qq_hi, qq_lo;
        measure_q_join(0, (uint64_t)sq, out_hi, out_lo);
        const uint64_t sums[3] = {(uint64_t)sqq, 0u, 0u};
        measure_qq_join(sums, qq_hi, qq_lo);
        CHECK(out_hi == 0 && out_lo == (uint64_t)sq && qq_hi == 0u && qq_lo == (uint64_t)sqq, "q = %llu", (unsigned long long)q);
    }
    CHECK(measure_scale(VK_FMT_R8_UNORM) == 255u && measure_scale(VK_FMT_R16_UNORM) == 65535u && measure_scale(VK_FMT_R16_FLOAT) == 16777216u, "the scales");
}

// ---- (4) ------------------------------------------------------------------------------------------------------------------------
static void check_run_sums() {
    for (uint64_t x = 0; x <= 130u; x++)
        for (uint64_t len = 1; x + len <= 130u; len++) {
            const uint64_t y = rnd_below(3u) ? rnd_below(2048u) : 0u, z = rnd_below(3u) ? rnd_below(2048u) : 0u;
            uint64_t s[9], want[9] = {};
            measure_run_sums(x, y, z, len, s);
            for (uint64_t k = 0; k < len; k++) {
                const uint64_t c[3] = {x + k, y, z};
                for (int a = 0; a < 3; a++) { want[a] += c[a]; want[3 + a] += c[a] * c[a]; }
                want[6] += c[0] * c[1]; want[7] += c[0] * c[2]; want[8] += c[1] * c[2];
            }
            for (int a = 0; a < 9; a++) CHECK(s[a] == want[a], "x %llu len %llu y %llu z %llu: sum %d", (unsigned long long)x, (unsigned long long)len, (unsigned long long)y, (unsigned long long)z, a);
        }
    // far out: a run at the end of a long row of a volume that just fits
    uint64_t s[9];
    measure_run_sums(2642000u, 0u, 0u, 64u, s);
    u128 want = 0;
    for (uint64_t k = 0; k < 64u; k++) want += (u128)(2642000u + k) * (2642000u + k);
    CHECK((u128)s[3] == want, "a run far out");
}

// ---- (5) ------------------------------------------------------------------------------------------------------------------------
static void gather(uint64_t *w, uint32_t k, uint64_t v) {
    CHECK(k < kMeasureWords, "word %u", k);
    switch (measure_word_op(k)) {
        case MOP_UMIN: w[k] = std::min(w[k], v); break;
        case MOP_UMAX: w[k] = std::max(w[k], v); break;
        case MOP_SMIN: w[k] = (uint64_t)std::min((int64_t)w[k], (int64_t)v); break;
        case MOP_SMAX: w[k] = (uint64_t)std::max((int64_t)w[k], (int64_t)v); break;
        default: w[k] += v; break;  // two's complement: a negative term wraps as the device's add does
    }
}
struct Run { uint32_t id, x, y, z, len; uint64_t i; };
struct Brute {
    u128 n = 0, sums[9] = {}, qq = 0, nonfinite = 0, faces[3] = {};
    i128 q = 0;
    uint64_t first = UINT64_MAX, lo[3] = {UINT64_MAX, UINT64_MAX, UINT64_MAX}, hi[3] = {};
    int64_t q_min = INT64_MAX, q_max = INT64_MIN;
};
static void check_records() {
    const uint32_t nx = 1u + rnd_below(rnd_below(3) ? 70u : 140u), ny = 1u + rnd_below(9u), nz = 1u + rnd_below(5u), regions = 1u + rnd_below(6u);
    const uint64_t n = (uint64_t)nx * ny * nz;
    std::vector<uint32_t> labels(n);
    std::vector<uint16_t> half(n);
    static const uint16_t special[] = {0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x8000, 0x0000, 0x7C00, 0xFC00, 0x7E00, 0x03FF, 0x3C00};
    uint32_t cur = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (rnd_below(4) == 0) cur = rnd_below(regions + 2u);  // ids above `regions` stand for "none": they become background
        labels[i] = cur <= regions ? cur : 0u;
        half[i] = rnd_below(3) ? (uint16_t)rnd() : special[rnd_below(sizeof special / sizeof special[0])];
    }
    auto label_at = [&](long x, long y, long z) -> uint32_t {
        if (x < 0 || y < 0 || z < 0 || x >= (long)nx || y >= (long)ny || z >= (long)nz) return 0u;
        return labels[(size_t)voxel_index((uint32_t)x, (uint32_t)y, (uint32_t)z, nx, ny)];
    };
    // voxel by voxel
    std::vector<Brute> want(regions);
    for (uint64_t i = 0; i < n; i++) {
        if (!labels[i]) continue;
        uint32_t c[3];
        label_coords((uint32_t)i, nx, ny, c[0], c[1], c[2]);
        Brute &b = want[labels[i] - 1u];
        b.n++;
        b.first = std::min(b.first, i);
        for (int a = 0; a < 3; a++) { b.lo[a] = std::min<uint64_t>(b.lo[a], c[a]); b.hi[a] = std::max<uint64_t>(b.hi[a], c[a] + 1u); b.sums[a] += c[a]; b.sums[3 + a] += (u128)c[a] * c[a]; }
        b.sums[6] += (u128)c[0] * c[1]; b.sums[7] += (u128)c[0] * c[2]; b.sums[8] += (u128)c[1] * c[2];
        bool finite;
        const int64_t q = measure_q_half(half[i], finite);
        if (finite) { b.q += q; b.qq += (u128)((i128)q * q); b.q_min = std::min(b.q_min, q); b.q_max = std::max(b.q_max, q); } else b.nonfinite++;
        for (int a = 0; a < 3; a++)
            for (int s = -1; s <= 1; s += 2) b.faces[a] += label_at((long)c[0] + (a == 0 ? s : 0), (long)c[1] + (a == 1 ? s : 0), (long)c[2] + (a == 2 ? s : 0)) != labels[i];
    }
    // run by run, as the kernel: a run ends where the label changes, where the row ends, and at random further places
    std::vector<Run> runs;
    for (uint64_t i = 0; i < n;) {
        uint32_t x, y, z;
        label_coords((uint32_t)i, nx, ny, x, y, z);
        uint32_t len = 1u;
        while (x + len < nx && labels[i + len] == labels[i] && len < 64u && rnd_below(9)) len++;
        if (labels[i]) runs.push_back(Run{labels[i], x, y, z, len, i});
        i += len;
    }
    for (size_t k = runs.size(); k > 1; k--) std::swap(runs[k - 1], runs[rnd_below((uint32_t)k)]);
    std::vector<uint64_t> words((size_t)regions * kMeasureWords);
    for (size_t e = 0; e < words.size(); e++) words[e] = measure_word_init((uint32_t)(e % kMeasureWords));
    for (const Run &r : runs) {
        uint64_t *w = words.data() + (size_t)(r.id - 1u) * kMeasureWords;
        gather(w, MW_N, r.len); gather(w, MW_FIRST, r.i);
        gather(w, MW_BOX_LO, r.x); gather(w, MW_BOX_LO + 1u, r.y); gather(w, MW_BOX_LO + 2u, r.z);
        gather(w, MW_BOX_HI, r.x + r.len - 1u); gather(w, MW_BOX_HI + 1u, r.y); gather(w, MW_BOX_HI + 2u, r.z);
        uint64_t s[9];
        measure_run_sums(r.x, r.y, r.z, r.len, s);
        for (uint32_t a = 0; a < 9u; a++) gather(w, MW_SUMS + a, s[a]);
        for (uint32_t k = 0; k < r.len; k++) {  // the run's lanes
            bool finite;
            const int64_t q = measure_q_half(half[r.i + k], finite);
            if (finite) {
                int64_t hi; uint64_t lo, limb[3];
                measure_q_split(q, hi, lo); measure_qq_split(q, limb);
                gather(w, MW_QMIN, (uint64_t)q); gather(w, MW_QMAX, (uint64_t)q);
                gather(w, MW_Q_HI, (uint64_t)hi); gather(w, MW_Q_LO, lo);
                gather(w, MW_QQ0, limb[0]); gather(w, MW_QQ1, limb[1]); gather(w, MW_QQ2, limb[2]);
            } else gather(w, MW_NONFINITE, 1u);
            for (int a = 0; a < 3; a++)
                for (int sgn = -1; sgn <= 1; sgn += 2)
                    gather(w, MW_FACES + (uint32_t)a, label_at((long)(r.x + k) + (a == 0 ? sgn : 0), (long)r.y + (a == 1 ? sgn : 0), (long)r.z + (a == 2 ? sgn : 0)) != r.id);
        }
    }
    for (uint32_t c = 0; c < regions; c++) {
        const vk_region g = measure_region(words.data() + (size_t)c * kMeasureWords);
        const Brute &b = want[c];
        CHECK(g.n_voxels == (uint64_t)b.n && g.first == b.first && g.n_nonfinite == (uint64_t)b.nonfinite && g.q_min == b.q_min && g.q_max == b.q_max, "region %u: counts and extremes", c + 1u);
        const uint32_t box[6] = {g.box.x0, g.box.y0, g.box.z0, g.box.x1, g.box.y1, g.box.z1};
        for (int a = 0; a < 3; a++) CHECK(box[a] == (b.n ? b.lo[a] : 0u) && box[3 + a] == (b.n ? b.hi[a] : 0u), "region %u: the box", c + 1u);
        const uint64_t sums[9] = {g.sum_x, g.sum_y, g.sum_z, g.sum_xx, g.sum_yy, g.sum_zz, g.sum_xy, g.sum_xz, g.sum_yz};
        for (int a = 0; a < 9; a++) CHECK((u128)sums[a] == b.sums[a], "region %u: index sum %d", c + 1u, a);
        CHECK(g.sum_q_lo == (uint64_t)b.q && g.sum_q_hi == (int64_t)(b.q >> 64), "region %u: sum_q", c + 1u);
        CHECK(g.sum_qq_lo == (uint64_t)b.qq && g.sum_qq_hi == (uint64_t)(b.qq >> 64), "region %u: sum_qq", c + 1u);
        for (int a = 0; a < 3; a++) CHECK((u128)g.faces[a] == b.faces[a], "region %u: faces across axis %d", c + 1u, a);
    }
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 100;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!g_state) g_state = 1;
    check_validation();
    check_overflow_bound();
    check_q_and_limbs();
    check_run_sums();
    for (int k = 0; k < cases; k++) check_records();
    std::printf("OK (%d cases)\n", cases);
    return 0;
}
