/* The rule of vk_volume_filter (include/vokselis_hip.h) restated in plain C, operation by operation in the stated
 * order: three whole-volume axis passes over f32 intermediates with clamped indices, the store rule of each format, and the 3x3x3
 * median as a sort of 27 keys.  Built with -ffp-contract=off; the one fused operation is the explicit fmaf.  Nothing here is shared with
 * the library's sources.
 *
 * fmt: 0 R8, 1 R16F, 3 R16_UNORM (the VK_FMT_ numbers).  op: 0 convolve, 1 median.  weights: [3][13].
 * kinds (added to): 0..5 taps whose index was clamped at the low / high end of x, y, z; 6 results whose clamped value lies exactly
 * between two integers (rint ties); 7 results clamped at 0, 8 at the top; 9 NaN outputs, 10 infinite outputs; 11 medians that tie with
 * the key below or above them. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TAPS 13

static float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    float f;
    if (e == 31u) {
        const uint32_t b = sign | 0x7f800000u | (m << 13);
        memcpy(&f, &b, 4);
        return f;
    }
    if (e == 0u) f = ldexpf((float)m, -24);
    else f = ldexpf((float)(m | 1024u), (int)e - 25);
    return sign ? -f : f;
}

/* round to nearest even, denormals kept, overflow to infinity, NaN to 0x7E00 */
static uint16_t float_to_half(float v) {
    if (v != v) return 0x7e00u;
    uint32_t b;
    memcpy(&b, &v, 4);
    const uint16_t sign = (uint16_t)((b >> 16) & 0x8000u);
    const double a = fabs((double)v);
    if (a == 0.0) return sign;
    if (isinf(v)) return (uint16_t)(sign | 0x7c00u);
    int ex;
    (void)frexp(a, &ex);                       /* a = f 2^ex, 0.5 <= f < 1: the leading bit is 2^(ex - 1) */
    int unit = ex - 1 - 10;                    /* the last place of a normal half with that leading bit */
    if (unit < -24) unit = -24;                /* denormals: the last place stays 2^-24 */
    const double q = nearbyint(ldexp(a, -unit));  /* exact scaling; ties to even in the default rounding mode */
    const double r = ldexp(q, unit);
    if (r >= 65520.0) return (uint16_t)(sign | 0x7c00u);
    if (r == 0.0) return sign;
    int e2;
    const double f2 = frexp(r, &e2);           /* r = f2 2^e2 */
    if (e2 - 1 < -14) return (uint16_t)(sign | (uint16_t)ldexp(r, 24));  /* a denormal: r / 2^-24 */
    const uint32_t mant = (uint32_t)ldexp(f2, 11) & 1023u, expo = (uint32_t)(e2 - 1 + 15);
    return (uint16_t)(sign | (expo << 10) | mant);
}

static uint32_t clampi(int64_t i, uint32_t n, uint64_t *lo, uint64_t *hi) {
    if (i < 0) { (*lo)++; return 0u; }
    if (i > (int64_t)n - 1) { (*hi)++; return n - 1u; }
    return (uint32_t)i;
}

static uint16_t half_key(uint16_t bits) { return (uint16_t)(bits ^ ((bits & 0x8000u) ? 0xffffu : 0x8000u)); }
static uint16_t half_unkey(uint16_t key) { return (uint16_t)(key ^ ((key & 0x8000u) ? 0x8000u : 0xffffu)); }

static int cmp_u32(const void *a, const void *b) {
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

int filter_restate(const void *in, void *out, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, int op, const uint32_t *radius, const float *weights, uint64_t *kinds) {
    const size_t n = (size_t)nx * ny * nz;
    const uint8_t *in8 = (const uint8_t *)in;
    const uint16_t *in16 = (const uint16_t *)in;
    uint8_t *out8 = (uint8_t *)out;
    uint16_t *out16 = (uint16_t *)out;
    const uint32_t dims[3] = {nx, ny, nz};
    if (fmt != 0 && fmt != 1 && fmt != 3) return 1;
    if (op == 1) {
        for (uint32_t z = 0; z < nz; z++)
            for (uint32_t y = 0; y < ny; y++)
                for (uint32_t x = 0; x < nx; x++) {
                    uint32_t k[27];
                    int c = 0;
                    uint64_t dummy = 0;
                    for (int dz = -1; dz <= 1; dz++)
                        for (int dy = -1; dy <= 1; dy++)
                            for (int dx = -1; dx <= 1; dx++) {
                                const uint32_t cx = clampi((int64_t)x + dx, nx, dy == 0 && dz == 0 ? &kinds[0] : &dummy, dy == 0 && dz == 0 ? &kinds[1] : &dummy);
                                const uint32_t cy = clampi((int64_t)y + dy, ny, dx == 0 && dz == 0 ? &kinds[2] : &dummy, dx == 0 && dz == 0 ? &kinds[3] : &dummy);
                                const uint32_t cz = clampi((int64_t)z + dz, nz, dx == 0 && dy == 0 ? &kinds[4] : &dummy, dx == 0 && dy == 0 ? &kinds[5] : &dummy);
                                const size_t i = (size_t)cx + (size_t)nx * ((size_t)cy + (size_t)ny * cz);
                                k[c++] = fmt == 0 ? in8[i] : (fmt == 1 ? half_key(in16[i]) : in16[i]);
                            }
                    qsort(k, 27, sizeof(uint32_t), cmp_u32);
                    if (k[12] == k[13] || k[14] == k[13]) kinds[11]++;
                    const size_t o = (size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * z);
                    if (fmt == 0) out8[o] = (uint8_t)k[13];
                    else out16[o] = fmt == 1 ? half_unkey((uint16_t)k[13]) : (uint16_t)k[13];
                }
        return 0;
    }
    if (op != 0) return 2;
    float *a = (float *)malloc((n ? n : 1) * sizeof(float)), *b = (float *)malloc((n ? n : 1) * sizeof(float));
    if (!a || !b) { free(a); free(b); return 3; }
    for (size_t i = 0; i < n; i++) a[i] = fmt == 0 ? (float)in8[i] : (fmt == 1 ? half_to_float(in16[i]) : (float)in16[i]);
    for (int axis = 0; axis < 3; axis++) {
        const uint32_t r = radius[axis];
        if (r == 0u) continue; /* skipped entirely: the weights are not read */
        const float *w = weights + TAPS * axis;
        const size_t stride = axis == 0 ? 1u : (axis == 1 ? (size_t)nx : (size_t)nx * ny);
        for (uint32_t z = 0; z < nz; z++)
            for (uint32_t y = 0; y < ny; y++)
                for (uint32_t x = 0; x < nx; x++) {
                    const uint32_t p[3] = {x, y, z};
                    const size_t o = (size_t)x + (size_t)nx * ((size_t)y + (size_t)ny * z);
                    const size_t base = o - (size_t)p[axis] * stride;
                    float acc = w[0] * a[base + (size_t)clampi((int64_t)p[axis] - (int64_t)r, dims[axis], &kinds[2 * axis], &kinds[2 * axis + 1]) * stride];
                    for (uint32_t k = 1; k <= 2u * r; k++)
                        acc = fmaf(w[k], a[base + (size_t)clampi((int64_t)p[axis] - (int64_t)r + (int64_t)k, dims[axis], &kinds[2 * axis], &kinds[2 * axis + 1]) * stride], acc);
                    b[o] = acc;
                }
        float *t = a;
        a = b;
        b = t;
    }
    for (size_t i = 0; i < n; i++) {
        const float v = a[i];
        if (fmt == 1) {
            const uint16_t h = float_to_half(v);
            if ((h & 0x7fffu) > 0x7c00u) kinds[9]++;
            else if ((h & 0x7fffu) == 0x7c00u) kinds[10]++;
            out16[i] = h;
        } else {
            const float top = fmt == 0 ? 255.0f : 65535.0f;
            if (v < 0.0f) kinds[7]++;
            if (v > top) kinds[8]++;
            const float c = fminf(fmaxf(v, 0.0f), top);
            if (c - floorf(c) == 0.5f) kinds[6]++;
            const float q = rintf(c);
            if (fmt == 0) out8[i] = (uint8_t)q;
            else out16[i] = (uint16_t)q;
        }
    }
    free(a);
    free(b);
    return 0;
}
