// TEST INFRASTRUCTURE: host build of the histogram's shared header (vokselis_amd/csrc/vk_hist.hpp) under ASan + UBSan, against brute force.
// 1. vk::hist_validate, the validation table of vk_volume_histogram: a NULL request, bins outside 1 .. 4096, lo or hi not finite, hi <= lo,
//    an unknown flag; an accepted request's constants are the double expressions rounded once.
// 2. vk::hist_bin is monotone in t -- below, bins 0 .. bins - 1, above, in that order -- for every bins from 1 to 4096; a NaN is HIST_NAN.
// 3. For random domains, hist_bin agrees with a long-double evaluation of (t / S - lo) bins / (hi - lo) wherever that lies further from
//    an integer than the roundings of k1, k2 and the fma can move it; +-inf land above / below, -0 at lo_k = 0 in bin 0; a k1 that overflows
//    yields a bin, never an undefined conversion.
// 4. vk::hist_key against `<` on all f16 values (sorted by key, the sequence must ascend, -0 directly below +0) and on random f32 pairs;
//    hist_key_value inverts it; hist_minmax_decode on the empty pair.
// 5. vk::voxel_clip_axis / voxel_clip_box against brute force over the voxel centres, (i + 0.5) / n in double within the closed interval.
// 6. vk::hist_window against a brute-force percentile of the sorted samples on small counts, and its refusals.
// 7. vk::hist_flush_passes: passes x voxels-per-pass stays within 2^32 - 1, one more pass would not.
// 8. vk::hist_grid, hist_runs (the runs enumerate exactly the box's voxels, each once), hist_run_chunks (no alignment makes a run touch
//    more chunks) and hist_cell_range (the bricks hold exactly the even cells the box needs) against brute force.
// usage: hist_fuzz <cases> <seed>; prints "OK (<cases> cases)" or the first violations, and exits non-zero on any.
#include "vk_hist.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

static uint64_t state;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static float unit() { return (float)((rnd() >> 40) / 16777216.0); }  // [0, 1)
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static long bad = 0;
static void fail(long c, const char *what, double a, double b) { if (bad < 10) printf("case %ld: %s (%a, %a)\n", c, what, a, b); bad++; }

static float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 31u) return from_bits(sign | 0x7f800000u | (m << 13));
    if (e != 0u) return from_bits(sign | ((e + 112u) << 23) | (m << 13));
    const float f = (float)m * 0x1p-24f;
    return sign ? -f : f;
}

static bool accepted(float lo, float hi, uint32_t bins, uint32_t flags) {
    vk_histogram h = {lo, hi, bins, flags};
    vk::HistConsts K;
    return vk::hist_validate(&h, vk::SCALE_R8, K) == nullptr;
}

static void check_validation(long c) {
    vk::HistConsts K;
    if (!vk::hist_validate(nullptr, vk::SCALE_R8, K)) fail(c, "a NULL request is accepted", 0, 0);
    if (!accepted(0.0f, 1.0f, 256, 0) || !accepted(0.0f, 1.0f, 1, VK_HIST_CLIP_BOX) || !accepted(-3.0e38f, 3.0e38f, 4096, 0) || !accepted(0.0f, 1.0e-45f, 7, 0))
        fail(c, "a plain request is refused", 0, 0);
    for (uint32_t b : {0u, 4097u, 5000u, 0x80000000u, 0xffffffffu})
        if (accepted(0.0f, 1.0f, b, 0)) fail(c, "bins outside 1 .. 4096 accepted", b, 0);
    for (float v : {NAN, INFINITY, -INFINITY}) {
        if (accepted(v, 1.0f, 16, 0)) fail(c, "lo not finite accepted", v, 0);
        if (accepted(0.0f, v, 16, 0)) fail(c, "hi not finite accepted", v, 0);
    }
    if (accepted(1.0f, 1.0f, 16, 0) || accepted(1.0f, 0.5f, 16, 0) || accepted(0.0f, -0.0f, 16, 0)) fail(c, "hi <= lo accepted", 0, 0);
    for (uint32_t f : {2u, 3u, 4u, 0x80000000u})
        if (accepted(0.0f, 1.0f, 16, f)) fail(c, "an unknown flag accepted", f, 0);
    const vk::SampleScale scales[3] = {vk::SCALE_VALUE, vk::SCALE_R8, vk::SCALE_U16};
    const double S[3] = {1.0, 255.0, 65535.0};
    for (int s = 0; s < 3; s++) {
        const float lo = (unit() - 0.5f) * 4.0f, hi = lo + unit() * 3.0f + 1e-3f;
        const uint32_t nb = 1u + (uint32_t)(rnd() % 4096u);
        vk_histogram h = {lo, hi, nb, 0};
        if (vk::hist_validate(&h, scales[s], K)) { fail(c, "a random request is refused", lo, hi); continue; }
        if (K.bins != nb || K.lo_k != (float)((double)lo * S[s]) || K.hi_k != (float)((double)hi * S[s]) ||
            K.k1 != (float)((double)nb / (((double)hi - (double)lo) * S[s])) || K.k2 != (float)(-(double)lo * (double)nb / ((double)hi - (double)lo)))
            fail(c, "the constants are not the double expressions rounded once", lo, hi);
    }
}

// below: -1, a bin: itself, above: bins -- the order a growing t must follow
static long rank_of(int b, uint32_t bins) { return b == vk::HIST_BELOW ? -1 : (b == vk::HIST_ABOVE ? (long)bins : (long)b); }

static void check_monotone() {
    for (uint32_t nb = 1; nb <= (uint32_t)VK_HIST_MAX_BINS; nb++) {
        const float lo = (unit() - 0.5f) * 2.0f, hi = lo + unit() + 1e-3f;
        vk_histogram h = {lo, hi, nb, 0};
        vk::HistConsts K;
        const vk::SampleScale sc = (nb % 3u) == 0u ? vk::SCALE_VALUE : ((nb % 3u) == 1u ? vk::SCALE_R8 : vk::SCALE_U16);
        if (vk::hist_validate(&h, sc, K)) { fail(0, "monotone: request refused", nb, 0); continue; }
        std::vector<float> t;
        const float span = K.hi_k - K.lo_k;
        for (int i = 0; i < 160; i++) t.push_back(K.lo_k + span * (unit() * 1.2f - 0.1f));
        for (float e : {K.lo_k, K.hi_k, nextafterf(K.lo_k, -INFINITY), nextafterf(K.hi_k, INFINITY), nextafterf(K.lo_k, INFINITY), nextafterf(K.hi_k, -INFINITY), -INFINITY, INFINITY}) t.push_back(e);
        std::sort(t.begin(), t.end());
        long prev = -1;
        for (float x : t) {
            const int b = vk::hist_bin(x, K.lo_k, K.hi_k, K.k1, K.k2, K.bins);
            if (b == vk::HIST_NAN || (b >= 0 && (uint32_t)b >= nb)) { fail(0, "monotone: a bin outside the range", nb, x); break; }
            const long r = rank_of(b, nb);
            if (r < prev) { fail(0, "hist_bin is not monotone in t", nb, x); break; }
            prev = r;
        }
        if (vk::hist_bin(K.lo_k, K.lo_k, K.hi_k, K.k1, K.k2, nb) < 0 || vk::hist_bin(K.hi_k, K.lo_k, K.hi_k, K.k1, K.k2, nb) < 0) fail(0, "an end of the domain is outside it", nb, 0);
        if (vk::hist_bin(NAN, K.lo_k, K.hi_k, K.k1, K.k2, nb) != vk::HIST_NAN || vk::hist_bin(-NAN, K.lo_k, K.hi_k, K.k1, K.k2, nb) != vk::HIST_NAN) fail(0, "a NaN is not HIST_NAN", nb, 0);
        if (vk::hist_slot(vk::HIST_NAN, nb) != nb || vk::hist_slot(vk::HIST_BELOW, nb) != nb + 1u || vk::hist_slot(vk::HIST_ABOVE, nb) != nb + 2u || vk::hist_slot((int)nb - 1, nb) != nb - 1u)
            fail(0, "hist_slot", nb, 0);
    }
}

static void check_bin_against_long_double(long c) {
    const vk::SampleScale scales[3] = {vk::SCALE_VALUE, vk::SCALE_R8, vk::SCALE_U16};
    const long double S[3] = {1.0L, 255.0L, 65535.0L};
    const int s = (int)(rnd() % 3u);
    const float lo = (unit() - 0.5f) * 8.0f, hi = lo + unit() * 4.0f + 1e-4f;
    const uint32_t nb = 1u + (uint32_t)(rnd() % 4096u);
    vk_histogram h = {lo, hi, nb, 0};
    vk::HistConsts K;
    if (vk::hist_validate(&h, scales[s], K)) { fail(c, "long double: request refused", lo, hi); return; }
    for (int i = 0; i < 200; i++) {
        const float t = K.lo_k + (K.hi_k - K.lo_k) * unit();
        if (!(t >= K.lo_k && t <= K.hi_k)) continue;
        const long double u = ((long double)t / S[s] - (long double)lo) * (long double)nb / ((long double)hi - (long double)lo);
        const long double tol = (fabsl((long double)t * (long double)K.k1) + fabsl((long double)K.k2) + fabsl(u) + 1.0L) * 0x1p-22L;
        if (fabsl(u - roundl(u)) <= tol) continue;  // too close to an edge to call
        long want = (long)floorl(u);
        want = want < 0 ? 0 : (want > (long)nb - 1 ? (long)nb - 1 : want);
        const int got = vk::hist_bin(t, K.lo_k, K.hi_k, K.k1, K.k2, nb);
        if ((long)got != want) fail(c, "hist_bin differs from the long-double evaluation away from an edge", t, (double)u);
    }
    if (vk::hist_bin(INFINITY, K.lo_k, K.hi_k, K.k1, K.k2, nb) != vk::HIST_ABOVE || vk::hist_bin(-INFINITY, K.lo_k, K.hi_k, K.k1, K.k2, nb) != vk::HIST_BELOW) fail(c, "an infinity is not above / below", 0, 0);
    {   // -0 at lo_k = 0 is bin 0; the identity's top value is the top bin
        vk_histogram id = {0.0f, 1.0f, 256, 0};
        vk::hist_validate(&id, vk::SCALE_R8, K);
        if (vk::hist_bin(-0.0f, K.lo_k, K.hi_k, K.k1, K.k2, 256) != 0 || vk::hist_bin(255.0f, K.lo_k, K.hi_k, K.k1, K.k2, 256) != 255) fail(c, "-0 or the top value of the identity", 0, 0);
    }
    {   // a domain a few denormals wide: k1 overflows, every t of the domain still gets a bin
        vk_histogram tiny = {0.0f, from_bits(1u + (uint32_t)(rnd() % 3u)), nb, 0};
        if (vk::hist_validate(&tiny, vk::SCALE_VALUE, K)) { fail(c, "a denormal domain is refused", 0, 0); return; }
        for (float t : {0.0f, -0.0f, tiny.hi, from_bits(1u)}) {
            if (!(t >= K.lo_k && t <= K.hi_k)) continue;
            const int b = vk::hist_bin(t, K.lo_k, K.hi_k, K.k1, K.k2, nb);
            if (b < 0 || (uint32_t)b >= nb) fail(c, "a denormal domain: a value of the domain has no bin", t, b);
        }
    }
}

static void check_key_f16() {
    std::vector<std::pair<uint32_t, float>> v;
    for (uint32_t h = 0; h < 65536u; h++) {
        const float f = half_to_float((uint16_t)h);
        if (f != f) continue;
        v.push_back({vk::hist_key(f), f});
        if (bits(vk::hist_key_value(vk::hist_key(f))) != bits(f)) fail(0, "hist_key_value does not invert hist_key", f, 0);
        if (vk::hist_key(f) == 0u || vk::hist_key(f) == 0xffffffffu) fail(0, "a non-NaN key collides with the empty marks", f, 0);
    }
    std::sort(v.begin(), v.end(), [](const std::pair<uint32_t, float> &a, const std::pair<uint32_t, float> &b) { return a.first < b.first; });
    for (size_t i = 1; i < v.size(); i++) {
        const float a = v[i - 1].second, b = v[i].second;
        if (v[i - 1].first == v[i].first) fail(0, "two f16 values share a key", a, b);
        const bool zeros = a == 0.0f && b == 0.0f && signbit(a) && !signbit(b);
        if (!(a < b) && !zeros) fail(0, "the key's order is not <'s on f16", a, b);
    }
    if (v.size() != 65536u - 2u * 1023u) fail(0, "f16 values walked", (double)v.size(), 0);
    float mn, mx;
    vk::hist_minmax_decode(0u, 0u, mn, mx);
    if (!(mn == INFINITY && mx == -INFINITY)) fail(0, "the empty pair does not decode to +inf, -inf", mn, mx);
    vk::hist_minmax_decode(~vk::hist_key(-0.0f), vk::hist_key(0.0f), mn, mx);
    if (bits(mn) != 0x80000000u || bits(mx) != 0u) fail(0, "min -0, max +0", mn, mx);
}

static void check_key_f32(long c) {
    for (int i = 0; i < 200; i++) {
        float a = from_bits((uint32_t)rnd()), b = (i & 1) ? from_bits(bits(a) + (uint32_t)(rnd() % 5u) - 2u) : from_bits((uint32_t)rnd());
        if (a != a || b != b) continue;
        if (a < b && !(vk::hist_key(a) < vk::hist_key(b))) fail(c, "a < b but key(a) >= key(b)", a, b);
        if (b < a && !(vk::hist_key(b) < vk::hist_key(a))) fail(c, "b < a but key(b) >= key(a)", a, b);
        if (bits(a) == bits(b) && vk::hist_key(a) != vk::hist_key(b)) fail(c, "equal values, different keys", a, b);
        if (bits(vk::hist_key_value(vk::hist_key(a))) != bits(a)) fail(c, "hist_key_value does not invert hist_key", a, 0);
    }
}

static void check_clip(long c) {
    const uint32_t n = 1u + (uint32_t)(rnd() % 70u);
    float lo, hi;
    switch (rnd() % 5u) {
        case 0: lo = unit(); hi = unit(); break;
        case 1: lo = (float)(rnd() % (n + 1u)) / (float)n; hi = (float)(rnd() % (n + 1u)) / (float)n; break;                       // on voxel faces
        case 2: lo = (float)(((double)(rnd() % n) + 0.5) / (double)n); hi = (float)(((double)(rnd() % n) + 0.5) / (double)n); break;  // on voxel centres, rounded to f32
        case 3: lo = 0.0f; hi = 1.0f; break;
        default: lo = unit(); hi = nextafterf(lo, 2.0f); break;                                                                   // between two centres, mostly
    }
    if (hi < lo) { const float t = lo; lo = hi; hi = t; }
    uint32_t i0, i1;
    vk::voxel_clip_axis(lo, hi, n, i0, i1);
    if (i0 > i1 || i1 > n) { fail(c, "clip axis: a range outside the axis", i0, i1); return; }
    uint32_t first = n, count = 0;
    for (uint32_t i = 0; i < n; i++) {
        const double ctr = ((double)i + 0.5) / (double)n;
        if (ctr >= (double)lo && ctr <= (double)hi) { if (first == n) first = i; count++; }
    }
    if (count != i1 - i0 || (count && first != i0)) fail(c, "clip axis differs from brute force over the centres", lo, hi);
    const float l3[3] = {lo, 0.0f, lo}, h3[3] = {hi, 1.0f, hi};
    const vk_voxel_box b = vk::voxel_clip_box(l3, h3, n, 5, n);
    if (b.x0 != i0 || b.x1 != i1 || b.y0 != 0u || b.y1 != 5u || b.z0 != i0 || b.z1 != i1 || !vk::voxel_box_ok(b, n, 5, n)) fail(c, "clip box", lo, hi);
    if (vk::voxel_box_voxels(b) != (uint64_t)(i1 - i0) * 5u * (uint64_t)(i1 - i0)) fail(c, "box voxels", 0, 0);
}

static void check_window(long c) {
    const uint32_t nb = 1u + (uint32_t)(rnd() % 40u);
    std::vector<uint64_t> counts(nb);
    std::vector<uint32_t> samples;
    for (uint32_t i = 0; i < nb; i++) {
        counts[i] = (rnd() % 3u) ? (rnd() % 6u) : 0u;
        for (uint64_t k = 0; k < counts[i]; k++) samples.push_back(i);
    }
    const float lo = (unit() - 0.5f) * 10.0f, hi = lo + unit() * 5.0f + 0.01f;
    double p_lo = (double)unit() * 0.6, p_hi = p_lo + (double)unit() * (1.0 - p_lo);
    if (rnd() % 4u == 0u) p_lo = 0.0;
    if (rnd() % 4u == 0u) p_hi = 1.0;
    float a = -1.0f, b = -2.0f;
    const char *why = vk::hist_window(counts.data(), nb, lo, hi, p_lo, p_hi, a, b);
    const size_t N = samples.size();
    if (N == 0 || !(p_lo < p_hi)) {
        if (!why || a != -1.0f || b != -2.0f) fail(c, "window: an empty histogram or empty percentile range accepted, or outputs touched", p_lo, p_hi);
        return;
    }
    const size_t r_lo = (size_t)floor(p_lo * (double)N);
    size_t r_hi = (size_t)ceil(p_hi * (double)N);
    if (r_hi > N) r_hi = N;
    const uint32_t b_lo = samples[r_lo < N ? r_lo : N - 1];
    uint32_t b_hi = samples[r_hi - 1];
    if (b_hi < b_lo) b_hi = b_lo;
    const float wa = (float)((double)lo + (double)b_lo * ((double)hi - (double)lo) / (double)nb), wb = (float)((double)lo + ((double)b_hi + 1.0) * ((double)hi - (double)lo) / (double)nb);
    if (!(wa < wb)) { if (!why) fail(c, "window: an empty rounded window accepted", wa, wb); return; }
    if (why || bits(a) != bits(wa) || bits(b) != bits(wb)) fail(c, "window differs from the sorted samples' percentiles", a, b);
}

static void check_window_refusals() {
    const uint64_t counts[4] = {1, 2, 0, 5}, zeros[4] = {0, 0, 0, 0};
    float a = 7.0f, b = 8.0f;
    auto refused = [&](const uint64_t *cn, uint32_t nb, float lo, float hi, double pl, double ph) {
        const char *why = vk::hist_window(cn, nb, lo, hi, pl, ph, a, b);
        return why != nullptr && a == 7.0f && b == 8.0f;
    };
    if (!refused(nullptr, 4, 0, 1, 0.1, 0.9) || !refused(zeros, 4, 0, 1, 0.1, 0.9) || !refused(counts, 0, 0, 1, 0.1, 0.9) || !refused(counts, 4097, 0, 1, 0.1, 0.9)) fail(0, "window refusals: counts / bins", 0, 0);
    if (!refused(counts, 4, 0, 1, -0.1, 0.9) || !refused(counts, 4, 0, 1, 0.5, 0.5) || !refused(counts, 4, 0, 1, 0.9, 0.1) || !refused(counts, 4, 0, 1, 0.1, 1.5) || !refused(counts, 4, 0, 1, NAN, 0.9) ||
        !refused(counts, 4, 0, 1, 0.1, NAN))
        fail(0, "window refusals: percentiles", 0, 0);
    if (!refused(counts, 4, 1, 1, 0.1, 0.9) || !refused(counts, 4, NAN, 1, 0.1, 0.9) || !refused(counts, 4, 0, INFINITY, 0.1, 0.9)) fail(0, "window refusals: domain", 0, 0);
    if (!refused(counts, 4, 1.0e30f, nextafterf(1.0e30f, INFINITY), 0.0, 0.1)) fail(0, "window refusals: a window that rounds to nothing", 0, 0);  // bin 0 of 4 over one ulp
    if (vk::hist_window(counts, 4, 0.0f, 1.0f, 0.0, 1.0, a, b) || a != 0.0f || b != 1.0f) fail(0, "the whole histogram's window is the domain", a, b);
    if (vk::hist_window(counts, 4, 0.0f, 1.0f, 0.5, 1.0, a, b) || a != 0.75f || b != 1.0f) fail(0, "the upper half of {1, 2, 0, 5}", a, b);
}

static void check_flush_and_grid(long c) {
    for (uint32_t vpp : {vk::hist_pass_voxels_linear(1), vk::hist_pass_voxels_linear(2), vk::hist_pass_voxels_cells(), 1u, 3u, 0xffffffffu, 1u + (uint32_t)(rnd() % 100000u)}) {
        const uint64_t p = vk::hist_flush_passes(vpp);
        if (p < 1u || p * vpp > vk::kHistFlushVoxels || (p + 1u) * vpp <= vk::kHistFlushVoxels) fail(c, "the flush bound", vpp, (double)p);
    }
    if (vk::hist_pass_voxels_linear(1) != 4096u || vk::hist_pass_voxels_linear(2) != 2048u || vk::hist_pass_voxels_cells() != 2048u || vk::kHistFlushVoxels != 0xffffffffull) fail(c, "voxels per pass", 0, 0);
    const uint64_t items = (rnd() % 3u) ? rnd() % 100000u : rnd() % (1ull << 40);
    const uint32_t per = (rnd() & 1u) ? 256u : 4u, cus = (uint32_t)(rnd() % 400u), cap = (rnd() & 1u) ? 0u : 1u + (uint32_t)(rnd() % 64u);
    const uint32_t g = vk::hist_grid(items, per, cus, cap);
    const uint64_t full = (uint64_t)(cus ? cus : 1u) * vk::kHistBlocksPerCU, need = (items + per - 1u) / per;
    uint64_t want = need < full ? need : full;
    if (cap && want > cap) want = cap;
    if (want < 1u) want = 1u;
    if (g != want || g < 1u || (cap && g > cap) || g > full) fail(c, "hist_grid", (double)items, g);
}

static void check_runs(long c) {
    const uint32_t nx = 1u + (uint32_t)(rnd() % 9u), ny = 1u + (uint32_t)(rnd() % 7u), nz = 1u + (uint32_t)(rnd() % 6u);
    vk_voxel_box b;
    auto range = [&](uint32_t n, uint32_t &a0, uint32_t &a1) {
        if (rnd() % 3u == 0u) { a0 = 0; a1 = n; return; }
        a0 = (uint32_t)(rnd() % (n + 1u)); a1 = (uint32_t)(rnd() % (n + 1u));
        if (a1 < a0) { const uint32_t t = a0; a0 = a1; a1 = t; }
    };
    range(nx, b.x0, b.x1); range(ny, b.y0, b.y1); range(nz, b.z0, b.z1);
    std::vector<int> want((size_t)nx * ny * nz, 0), got(want.size(), 0);
    for (uint32_t z = b.z0; z < b.z1; z++)
        for (uint32_t y = b.y0; y < b.y1; y++)
            for (uint32_t x = b.x0; x < b.x1; x++) want[x + (size_t)nx * (y + (size_t)ny * z)]++;
    if (vk::voxel_box_voxels(b) != 0u) {
        const vk::HistRuns R = vk::hist_runs(b, nx, ny);
        if ((uint64_t)R.len * R.na * R.nb != vk::voxel_box_voxels(b)) fail(c, "runs: the runs do not hold the box's voxel count", R.len, R.na);
        for (uint32_t rb = 0; rb < R.nb; rb++)
            for (uint32_t ra = 0; ra < R.na; ra++)
                for (uint64_t k = 0; k < R.len; k++) {
                    const uint64_t i = R.off0 + ra * R.sa + rb * R.sb + k;
                    if (i >= got.size()) { fail(c, "runs: a voxel outside the volume", (double)i, 0); return; }
                    got[i]++;
                }
        if (got != want) fail(c, "runs: not exactly the box's voxels, each once", nx, ny);
        if (b.x0 == 0u && b.x1 == nx && b.y0 == 0u && b.y1 == ny && (R.na != 1u || R.nb != 1u)) fail(c, "runs: full planes did not merge into one run", 0, 0);
        for (uint32_t elem : {1u, 2u})
            for (uint64_t start = 0; start < 16u; start++) {  // whatever the alignment of the run's first byte
                const uint64_t byte0 = start * elem, byte1 = byte0 + R.len * elem;
                const uint64_t touched = (byte1 + 15u) / 16u - byte0 / 16u;
                if (touched > vk::hist_run_chunks(R.len, elem)) fail(c, "a run touches more chunks than hist_run_chunks", (double)R.len, (double)start);
            }
    }
    // cells: the bricks of even cells
    uint32_t b0, nb;
    const uint32_t x0 = b.x0, x1 = b.x1;
    vk::hist_cell_range(x0, x1, b0, nb);
    if (x1 > x0) {
        for (uint32_t x = x0; x < x1; x++) {
            const uint32_t brick = (x >> 1) >> 1;  // voxel x lies in even cell x >> 1, two even cells to a brick
            if (brick < b0 || brick >= b0 + nb) fail(c, "cell range: a voxel's brick is outside the range", x, b0);
        }
        if (b0 != x0 >> 2 || b0 + nb - 1u != (x1 - 1u) >> 2) fail(c, "cell range: a brick without a voxel of the box", x0, x1);
    } else if (nb != 0u) fail(c, "cell range: an empty range has bricks", x0, x1);
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 300;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!state) state = 1;
    check_monotone();
    check_key_f16();
    check_window_refusals();
    for (long c = 0; c < cases; c++) {
        check_validation(c);
        check_bin_against_long_double(c);
        check_key_f32(c);
        check_clip(c);
        check_window(c);
        check_flush_and_grid(c);
        check_runs(c);
    }
    if (bad) { printf("%ld violations\n", bad); return 1; }
    printf("OK (%ld cases)\n", cases);
    return 0;
}
