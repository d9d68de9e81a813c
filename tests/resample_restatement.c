/* The rule of vk_volume_resample, restated from the comment in include/vokselis_hip.h alone: plain loops over the output voxels, every
 * index, fraction and weight recomputed per voxel -- no tables, nothing shared with vokselis_amd/csrc.  Built by the tests with
 * -ffp-contract=off, so that fmaf is fused where written and nowhere else.
 * Formats: 0 R8_UNORM, 1 R16_FLOAT, 3 R16_UNORM.  Modes: 0 NEAREST, 1 LINEAR, 2 AREA. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float half_value(uint16_t h) {
    const int s = h >> 15, e = (h >> 10) & 31, m = h & 1023;
    double v;
    if (e == 31) v = m ? (double)NAN : (double)INFINITY;
    else if (e == 0) v = ldexp((double)m, -24);
    else v = ldexp((double)(1024 + m), e - 25);
    return (float)(s ? -v : v);
}

/* f32 -> f16: round to nearest even, subnormals kept, overflow to infinity, any NaN 0x7E00 */
static uint16_t half_bits(float v) {
    if (v != v) return 0x7e00;
    const uint16_t sign = signbit(v) ? 0x8000 : 0;
    const double a = fabs((double)v);
    if (a >= 65520.0) return sign | 0x7c00; /* the midpoint between 65504 and 2^16 is a tie to the even side: infinity */
    if (a < ldexp(1.0, -14)) return sign | (uint16_t)rint(a * 16777216.0); /* multiples of 2^-24; 1024 of them are the smallest normal */
    int e;
    const double m = frexp(a, &e); /* a = m 2^e, 0.5 <= m < 1 */
    int mant = (int)rint((2.0 * m - 1.0) * 1024.0), ex = e - 1 + 15;
    if (mant == 1024) { mant = 0; ex++; }
    return sign | (uint16_t)(ex << 10) | (uint16_t)mant;
}

static double scale_of(int fmt) { return fmt == 0 ? 255.0 : (fmt == 3 ? 65535.0 : 1.0); }

typedef struct {
    const void *vol;
    uint32_t nx, ny, nz;
    int fmt;
    int64_t x0, y0, z0, bx, by, bz; /* the box: its low corner and extents */
} Source;

static int64_t clampi(int64_t i, int64_t n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }
static int64_t floordiv(int64_t a, int64_t b) { int64_t q = a / b; if ((a % b != 0) && ((a < 0) != (b < 0))) q--; return q; }

/* the stored bits of box voxel (i, j, k), indices clamped to the box */
static uint16_t stored(const Source *s, int64_t i, int64_t j, int64_t k) {
    const uint64_t x = (uint64_t)(s->x0 + clampi(i, s->bx)), y = (uint64_t)(s->y0 + clampi(j, s->by)), z = (uint64_t)(s->z0 + clampi(k, s->bz));
    const uint64_t at = x + (uint64_t)s->nx * (y + (uint64_t)s->ny * z);
    return s->fmt == 0 ? ((const uint8_t *)s->vol)[at] : ((const uint16_t *)s->vol)[at];
}
static float texel(const Source *s, int64_t i, int64_t j, int64_t k) {
    const uint16_t b = stored(s, i, j, k);
    return s->fmt == 1 ? half_value(b) : (float)b;
}

static float lerp(float a, float b, float f) { return f == 0.0f ? a : fmaf(f, b - a, a); }

static void linear_axis(int64_t j, int64_t nb, int64_t n, int64_t *i, float *f) {
    const int64_t num = (2 * j + 1) * nb - n, den = 2 * n;
    *i = floordiv(num, den);
    *f = (float)((double)(num - *i * den) / (double)den);
}

static int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
static int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
static float area_weight(int64_t j, int64_t k, int64_t nb, int64_t n) {
    const int64_t o = min64((j + 1) * nb, (k + 1) * n) - max64(j * nb, k * n);
    return (float)((double)o / (double)nb);
}

static float area_value(const Source *s, int64_t jx, int64_t jy, int64_t jz, int64_t nx, int64_t ny, int64_t nz) {
    const int64_t kx0 = floordiv(jx * s->bx, nx), kx1 = floordiv((jx + 1) * s->bx - 1, nx);
    const int64_t ky0 = floordiv(jy * s->by, ny), ky1 = floordiv((jy + 1) * s->by - 1, ny);
    const int64_t kz0 = floordiv(jz * s->bz, nz), kz1 = floordiv((jz + 1) * s->bz - 1, nz);
    float az = 0.0f;
    for (int64_t kz = kz0; kz <= kz1; kz++) {
        float ay = 0.0f;
        for (int64_t ky = ky0; ky <= ky1; ky++) {
            float ax = 0.0f;
            for (int64_t kx = kx0; kx <= kx1; kx++) { /* the x reduction of row (ky, kz) */
                const float w = area_weight(jx, kx, s->bx, nx), t = texel(s, kx, ky, kz);
                ax = kx == kx0 ? w * t : fmaf(w, t, ax);
            }
            const float w = area_weight(jy, ky, s->by, ny); /* the y reduction over the x results */
            ay = ky == ky0 ? w * ax : fmaf(w, ax, ay);
        }
        const float w = area_weight(jz, kz, s->bz, nz); /* the z reduction over the y results */
        az = kz == kz0 ? w * ay : fmaf(w, ay, az);
    }
    return az;
}

static uint16_t store(float v, int fmt) {
    if (fmt == 1) return half_bits(v);
    const float top = fmt == 0 ? 255.0f : 65535.0f;
    if (v != v) return 0;
    return (uint16_t)rintf(fminf(fmaxf(v, 0.0f), top));
}

/* box: x0, y0, z0, x1, y1, z1.  dims: the output extents, all > 0.  window: 0 / 1.  out: dims[0] dims[1] dims[2] elements of fmt_out, x
 * fastest.  Returns 0, or 1 for what the library refuses (the AREA ratio, a bad window). */
int resample_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt_in, const uint32_t *box, int mode, const uint32_t *dims, int fmt_out, int window,
                     float lo, float hi, void *out) {
    Source s = {vol, nx, ny, nz, fmt_in, box[0], box[1], box[2], (int64_t)box[3] - box[0], (int64_t)box[4] - box[1], (int64_t)box[5] - box[2]};
    const int64_t ox = dims[0], oy = dims[1], oz = dims[2];
    if (s.bx <= 0 || s.by <= 0 || s.bz <= 0 || ox <= 0 || oy <= 0 || oz <= 0) return 1;
    if (mode == 2 && (s.bx > 16 * ox || s.by > 16 * oy || s.bz > 16 * oz)) return 1;
    const int map = fmt_out != fmt_in || window;
    float a = 1.0f, b = 0.0f;
    if (map) {
        const double l = window ? (double)lo : 0.0, h = window ? (double)hi : 1.0;
        if (!(l < h)) return 1;
        a = (float)(scale_of(fmt_out) / ((h - l) * scale_of(fmt_in)));
        b = (float)(-l * scale_of(fmt_out) / (h - l));
        if (!isfinite(a) || !isfinite(b)) return 1;
    }
    for (int64_t jz = 0; jz < oz; jz++)
        for (int64_t jy = 0; jy < oy; jy++)
            for (int64_t jx = 0; jx < ox; jx++) {
                uint16_t bits;
                float v;
                if (mode == 0) {
                    const int64_t ix = floordiv((2 * jx + 1) * s.bx, 2 * ox), iy = floordiv((2 * jy + 1) * s.by, 2 * oy), iz = floordiv((2 * jz + 1) * s.bz, 2 * oz);
                    bits = stored(&s, ix, iy, iz);
                    v = texel(&s, ix, iy, iz);
                } else if (mode == 1) {
                    int64_t ix, iy, iz;
                    float fx, fy, fz;
                    linear_axis(jx, s.bx, ox, &ix, &fx);
                    linear_axis(jy, s.by, oy, &iy, &fy);
                    linear_axis(jz, s.bz, oz, &iz, &fz);
                    const float l00 = lerp(texel(&s, ix, iy, iz), texel(&s, ix + 1, iy, iz), fx);
                    const float l10 = lerp(texel(&s, ix, iy + 1, iz), texel(&s, ix + 1, iy + 1, iz), fx);
                    const float l01 = lerp(texel(&s, ix, iy, iz + 1), texel(&s, ix + 1, iy, iz + 1), fx);
                    const float l11 = lerp(texel(&s, ix, iy + 1, iz + 1), texel(&s, ix + 1, iy + 1, iz + 1), fx);
                    const float m0 = lerp(l00, l10, fy), m1 = lerp(l01, l11, fy);
                    v = lerp(m0, m1, fz);
                    bits = 0;
                } else {
                    v = area_value(&s, jx, jy, jz, ox, oy, oz);
                    bits = 0;
                }
                if (map) v = fmaf(a, v, b);
                if (mode != 0 || map) bits = store(v, fmt_out);
                const uint64_t at = (uint64_t)jx + (uint64_t)ox * ((uint64_t)jy + (uint64_t)oy * (uint64_t)jz);
                if (fmt_out == 0) ((uint8_t *)out)[at] = (uint8_t)bits;
                else ((uint16_t *)out)[at] = bits;
            }
    return 0;
}
