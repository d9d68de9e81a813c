/* The rule of vk_volume_histogram (include/vokselis_hip.h) written out over the dense array: one walk of the voxel
 * box in x-fastest order, the classification with its operations in the specification's order (-ffp-contract=off; fmaf for the one fused
 * operation), min and max in the order in which -0 lies below +0, the sums in f64 in the order of the walk.  Independent of the library:
 * it includes none of its headers.  Beside the result it counts the voxels of each kind the case list must contain. */
#include <math.h>
#include <stdint.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3 };
enum { KIND_NAN = 0, KIND_BELOW, KIND_ABOVE, KIND_AT_LO, KIND_AT_HI, KIND_TOP_CLAMPED, KIND_NEG_ZERO, KIND_COUNT };

static float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31u, m = h & 1023u;
    uint32_t bits;
    float f;
    if (e == 31u) bits = sign | 0x7f800000u | (m << 13);
    else if (e != 0u) bits = sign | ((e + 112u) << 23) | (m << 13);
    else if (m == 0u) bits = sign;
    else {
        f = (float)m * 0x1p-24f; /* a subnormal half: exact */
        return sign ? -f : f;
    }
    memcpy(&f, &bits, 4);
    return f;
}

/* a < b in the order of min and max: the usual order, and -0 below +0 */
static int below(float a, float b) {
    if (a < b) return 1;
    if (a == b && a == 0.0f) return signbit(a) && !signbit(b);
    return 0;
}

/* box: x0, y0, z0, x1, y1, z1.  counts: bins entries; cats: n_nan, n_below, n_above, n_finite; sums: sum, sum_sq; minmax: min, max;
 * kinds: KIND_COUNT entries, added to. */
int hist_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, const uint32_t *box, float lo_k, float hi_k, float k1, float k2,
                 uint32_t bins, uint64_t *counts, uint64_t *cats, double *sums, float *minmax, uint64_t *kinds) {
    float mn = INFINITY, mx = -INFINITY;
    double sum = 0.0, sum_sq = 0.0;
    if (box[0] > box[3] || box[1] > box[4] || box[2] > box[5] || box[3] > nx || box[4] > ny || box[5] > nz || bins < 1u) return 1;
    memset(counts, 0, sizeof(uint64_t) * bins);
    memset(cats, 0, sizeof(uint64_t) * 4);
    for (uint32_t z = box[2]; z < box[5]; z++)
        for (uint32_t y = box[1]; y < box[4]; y++)
            for (uint32_t x = box[0]; x < box[3]; x++) {
                const size_t i = (size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * (size_t)z);
                float t;
                if (fmt == FMT_U8) t = (float)((const uint8_t *)vol)[i];
                else if (fmt == FMT_U16) t = (float)((const uint16_t *)vol)[i];
                else t = half_to_float(((const uint16_t *)vol)[i]);
                if (isnan(t)) { cats[0]++; kinds[KIND_NAN]++; continue; }
                if (below(t, mn)) mn = t;
                if (below(mx, t)) mx = t;
                if (isfinite(t)) {
                    const double d = (double)t;
                    cats[3]++;
                    sum = sum + d;
                    sum_sq = sum_sq + d * d;
                }
                if (t < lo_k) { cats[1]++; kinds[KIND_BELOW]++; continue; }
                if (t > hi_k) { cats[2]++; kinds[KIND_ABOVE]++; continue; }
                {
                    const float u = floorf(fmaf(t, k1, k2));
                    int64_t b = (int64_t)u; /* finite here: the cases keep k1 and k2 finite */
                    if (b > (int64_t)bins - 1) { b = (int64_t)bins - 1; kinds[KIND_TOP_CLAMPED]++; }
                    if (b < 0) b = 0;
                    counts[b]++;
                    if (t == lo_k) kinds[KIND_AT_LO]++;
                    if (t == hi_k) kinds[KIND_AT_HI]++;
                    if (t == 0.0f && signbit(t)) kinds[KIND_NEG_ZERO]++;
                }
            }
    sums[0] = sum;
    sums[1] = sum_sq;
    minmax[0] = mn;
    minmax[1] = mx;
    return 0;
}
