/* vk_local_thickness restated from the rule in include/vokselis_hip.h in plain sequential C, as a scatter: every voxel u of S is the
 * centre of a ball, and the ball paints its capped squared radius Dc(u) onto every voxel v of S with d2(u, v) < Dc(u) that holds less.
 * D comes from this file's own distance -- one axis at a time, every entry of a line against ALL entries of the line, as
 * dist_restatement.c does it -- and not from the library.  No tiles, no skips, no lists.  Built with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3 };
#define D2_INF 0xFFFFFFFFu

static float half_value(uint16_t h) {
    const uint32_t sign = (uint32_t)(h >> 15), e = (h >> 10) & 31u, m = h & 1023u;
    float v;
    if (e == 31u) v = m ? NAN : INFINITY;
    else if (e == 0u) v = ldexpf((float)m, -24);
    else v = ldexpf((float)(m | 1024u), (int)e - 25);
    return sign ? -v : v;
}

/* f32 -> f16, round to nearest even, denormals kept, overflow to infinity (the value is finite) */
static uint16_t half_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const float a = fabsf(f);
    if (a == 0.0f) return sign;
    int ex;
    (void)frexpf(a, &ex);
    int q = ex - 11;
    if (q < -24) q = -24;
    const float r = rintf(ldexpf(a, -q));
    const float back = ldexpf(r, q);
    if (back >= 65520.0f) return (uint16_t)(sign | 0x7c00u);
    if (back < 6.103515625e-05f) return (uint16_t)(sign | (uint16_t)r);
    int e2;
    const float m2 = frexpf(back, &e2);
    return (uint16_t)(sign | (uint16_t)(((e2 + 14) << 10) | ((uint32_t)ldexpf(m2, 11) & 1023u)));
}

static float texel(const void *vol, uint64_t i, int fmt) {
    if (fmt == FMT_U8) return (float)((const uint8_t *)vol)[i];
    if (fmt == FMT_U16) return (float)((const uint16_t *)vol)[i];
    return half_value(((const uint16_t *)vol)[i]);
}

/* F: a value through the store rule of the three formats */
static uint32_t store_bits(float v, int fmt) {
    if (fmt == FMT_F16) return half_bits(v);
    const float top = fmt == FMT_U8 ? 255.0f : 65535.0f;
    return (uint32_t)rintf(fminf(fmaxf(v * top, 0.0f), top));
}

/* d[v] = D2(A, v) for the set A = { v : in[v] != 0 }: INF when A is empty */
static void distance_to(const uint8_t *in, const uint32_t *dims, const uint32_t *spacing, uint32_t *d, uint64_t *cur, uint64_t *nxt) {
    const uint64_t n = (uint64_t)dims[0] * dims[1] * dims[2];
    const uint64_t none = UINT64_MAX;
    const uint64_t stride[3] = {1u, dims[0], (uint64_t)dims[0] * dims[1]};
    for (uint64_t i = 0; i < n; i++) cur[i] = in[i] ? 0u : none;
    for (int axis = 0; axis < 3; axis++) {
        const uint32_t len = dims[axis];
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t at = (uint32_t)(i / stride[axis] % len);
            const uint64_t line = i - (uint64_t)at * stride[axis];
            uint64_t best = none;
            for (uint32_t j = 0; j < len; j++) {
                const uint64_t g = cur[line + (uint64_t)j * stride[axis]];
                if (g == none) continue;
                const uint64_t off = (uint64_t)spacing[axis] * (uint64_t)(at > j ? at - j : j - at);
                if (g + off * off < best) best = g + off * off;
            }
            nxt[i] = best;
        }
        uint64_t *t = cur; cur = nxt; nxt = t;
    }
    for (uint64_t i = 0; i < n; i++) d[i] = cur[i] == none ? D2_INF : (uint32_t)cur[i];
}

/* vol: nx ny nz texels.  box: 6.  spacing: 3.  t2: nx ny nz uint32.  dense: nx ny nz texels.  gain: 0 asks for the automatic one.
 * result: n_foreground, max_t2, n_saturated, sum_t2, the bits of the gain used.  Returns 0, -1 when memory runs out, -2 when a squared
 * distance might not fit (the header's VK_ERR_UNSUPPORTED). */
int thick_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, float lo, float hi, const uint32_t *spacing, float max_radius, float gain, float fill_out,
                  const uint32_t *box, uint32_t *t2, void *dense, uint64_t *result) {
    const uint32_t dims[3] = {nx, ny, nz};
    const uint64_t n = (uint64_t)nx * ny * nz;
    long double bound = 0.0L;
    for (int c = 0; c < 3; c++) {
        const long double a = (long double)spacing[c] * (long double)(dims[c] - 1u);
        bound += a * a;
    }
    if (bound > (long double)0xFFFFFFFEu) return -2;
    const float lo_k = fmt == FMT_U8 ? lo * 255.0f : (fmt == FMT_U16 ? lo * 65535.0f : lo);
    const float hi_k = fmt == FMT_U8 ? hi * 255.0f : (fmt == FMT_U16 ? hi * 65535.0f : hi);
    const uint64_t cap = (uint64_t)floor((double)max_radius * (double)max_radius);
    uint8_t *s = calloc(n, 1), *a = calloc(n, 1);
    uint32_t *d = malloc(n * sizeof *d);
    uint64_t *t0 = malloc(n * sizeof *t0), *t1 = malloc(n * sizeof *t1);
    if (!s || !a || !d || !t0 || !t1) { free(s); free(a); free(d); free(t0); free(t1); return -1; }
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = (uint32_t)(i % nx), y = (uint32_t)(i / nx % ny), z = (uint32_t)(i / ((uint64_t)nx * ny));
        const float t = texel(vol, i, fmt);
        s[i] = x >= box[0] && x < box[3] && y >= box[1] && y < box[4] && z >= box[2] && z < box[5] && t >= lo_k && t <= hi_k;
        a[i] = !s[i];
    }
    distance_to(a, dims, spacing, d, t0, t1);
    memset(t2, 0, n * sizeof *t2);
    for (uint32_t uz = 0; uz < nz; uz++)
        for (uint32_t uy = 0; uy < ny; uy++)
            for (uint32_t ux = 0; ux < nx; ux++) {
                const uint64_t iu = ux + (uint64_t)nx * (uy + (uint64_t)ny * uz);
                if (!s[iu]) continue;
                const uint64_t dc = (uint64_t)d[iu] < cap ? (uint64_t)d[iu] : cap;  /* INF > cap */
                /* the box of the ball: (w k)^2 < dc along each axis */
                int64_t r[3];
                for (int c = 0; c < 3; c++) {
                    int64_t k = 0;
                    while ((uint64_t)spacing[c] * (uint64_t)(k + 1) * ((uint64_t)spacing[c] * (uint64_t)(k + 1)) < dc) k++;
                    r[c] = k;
                }
                for (int64_t vz = (int64_t)uz - r[2]; vz <= (int64_t)uz + r[2]; vz++) {
                    if (vz < 0 || vz >= (int64_t)nz) continue;
                    for (int64_t vy = (int64_t)uy - r[1]; vy <= (int64_t)uy + r[1]; vy++) {
                        if (vy < 0 || vy >= (int64_t)ny) continue;
                        for (int64_t vx = (int64_t)ux - r[0]; vx <= (int64_t)ux + r[0]; vx++) {
                            if (vx < 0 || vx >= (int64_t)nx) continue;
                            const uint64_t iv = (uint64_t)vx + (uint64_t)nx * ((uint64_t)vy + (uint64_t)ny * (uint64_t)vz);
                            if (!s[iv]) continue;
                            const int64_t ex = (int64_t)spacing[0] * (vx - (int64_t)ux), ey = (int64_t)spacing[1] * (vy - (int64_t)uy), ez = (int64_t)spacing[2] * (vz - (int64_t)uz);
                            if ((uint64_t)(ex * ex + ey * ey + ez * ez) < dc && (uint64_t)t2[iv] < dc) t2[iv] = (uint32_t)dc;
                        }
                    }
                }
            }
    memset(result, 0, 5 * sizeof *result);
    for (uint64_t i = 0; i < n; i++) {
        result[0] += s[i];
        if (t2[i] > result[1]) result[1] = t2[i];
        result[2] += s[i] && (uint64_t)t2[i] == cap;
        result[3] += t2[i];
    }
    if (gain == 0.0f) gain = result[1] ? 1.0f / sqrtf((float)result[1]) : 0.0f;
    uint32_t gbits;
    memcpy(&gbits, &gain, 4);
    result[4] = gbits;
    const uint32_t f_out = store_bits(fill_out, fmt);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t bits = f_out;
        if (s[i]) {
            const float root = sqrtf((float)t2[i]);
            const float w = root * gain;
            bits = store_bits(w, fmt);
        }
        if (fmt == FMT_U8) ((uint8_t *)dense)[i] = (uint8_t)bits;
        else ((uint16_t *)dense)[i] = (uint16_t)bits;
    }
    free(s); free(a); free(d); free(t0); free(t1);
    return 0;
}
