/* vk_distance_transform restated from the rule in include/vokselis_hip.h in plain sequential C.  The squared distance to a set is built
 * one axis at a time -- x, then y, then z -- and along a line every entry takes the minimum over ALL entries of the line of their value
 * plus the squared offset: a quadratic inner loop, no envelope, no stack, no division.  Morphology thresholds that distance, once or
 * twice, exactly as the header composes dil and ero.  Shares nothing with the library's line function.  Built with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3 };
enum { OP_OUTSIDE = 0, OP_INSIDE = 1, OP_DILATE = 2, OP_ERODE = 3, OP_CLOSE = 4, OP_OPEN = 5 };
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

/* F: a fill through the store rule of the three formats */
static uint32_t fill_bits(float fill, int fmt) {
    if (fmt == FMT_F16) return half_bits(fill);
    const float top = fmt == FMT_U8 ? 255.0f : 65535.0f;
    return (uint32_t)rintf(fminf(fmaxf(fill * top, 0.0f), top));
}

/* d2[v] = D2(A, v) for the set A = { v : in[v] != 0 }: INF when A is empty.  tmp: n words. */
static void distance_to(const uint8_t *in, const uint32_t *dims, const uint32_t *spacing, uint32_t *d2, uint64_t *cur, uint64_t *nxt) {
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
    for (uint64_t i = 0; i < n; i++) d2[i] = cur[i] == none ? D2_INF : (uint32_t)cur[i];
}

/* vol: nx ny nz texels.  box: 6.  spacing: 3.  d2: nx ny nz uint32 (written by the distance ops).  dense: nx ny nz texels (written by the
 * morphology ops).  result: n_foreground, n_result, n_added, n_removed, max_d2.  Returns 0, -1 when memory runs out, -2 when a squared
 * distance might not fit (the header's VK_ERR_UNSUPPORTED). */
int dist_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, float lo, float hi, int op, const uint32_t *spacing, float radius, float fill_in, float fill_out,
                 const uint32_t *box, uint32_t *d2, void *dense, uint64_t *result) {
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
    const uint64_t r2 = (uint64_t)floor((double)radius * (double)radius);
    uint8_t *s = calloc(n, 1), *a = calloc(n, 1), *m = calloc(n, 1);
    uint32_t *d = malloc(n * sizeof *d);
    uint64_t *t0 = malloc(n * sizeof *t0), *t1 = malloc(n * sizeof *t1);
    if (!s || !a || !m || !d || !t0 || !t1) { free(s); free(a); free(m); free(d); free(t0); free(t1); return -1; }
    uint64_t n_s = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = (uint32_t)(i % nx), y = (uint32_t)(i / nx % ny), z = (uint32_t)(i / ((uint64_t)nx * ny));
        const float t = texel(vol, i, fmt);
        s[i] = x >= box[0] && x < box[3] && y >= box[1] && y < box[4] && z >= box[2] && z < box[5] && t >= lo_k && t <= hi_k;
        n_s += s[i];
    }
    memset(result, 0, 5 * sizeof *result);
    result[0] = n_s;
    if (op == OP_OUTSIDE || op == OP_INSIDE) {
        for (uint64_t i = 0; i < n; i++) a[i] = op == OP_OUTSIDE ? s[i] : !s[i];
        distance_to(a, dims, spacing, d2, t0, t1);
        result[1] = n_s;
        for (uint64_t i = 0; i < n; i++)
            if (d2[i] != D2_INF && d2[i] > result[4]) result[4] = d2[i];
    } else {
        /* dil(A) = { D2(A, v) <= R2 }; ero(A) = { D2(not A, v) > R2 } */
        memcpy(m, s, n);
        const int steps = op == OP_CLOSE || op == OP_OPEN ? 2 : 1;
        for (int k = 0; k < steps; k++) {
            const int dilate = op == OP_DILATE || (op == OP_CLOSE && k == 0) || (op == OP_OPEN && k == 1);
            for (uint64_t i = 0; i < n; i++) a[i] = dilate ? m[i] : !m[i];
            distance_to(a, dims, spacing, d, t0, t1);
            for (uint64_t i = 0; i < n; i++) m[i] = dilate ? (d[i] != D2_INF && (uint64_t)d[i] <= r2) : (d[i] == D2_INF || (uint64_t)d[i] > r2);
        }
        const uint32_t f_in = fill_bits(fill_in, fmt), f_out = fill_bits(fill_out, fmt);
        for (uint64_t i = 0; i < n; i++) {
            result[1] += m[i];
            result[2] += m[i] && !s[i];
            result[3] += s[i] && !m[i];
            if (fmt == FMT_U8) ((uint8_t *)dense)[i] = m[i] == s[i] ? ((const uint8_t *)vol)[i] : (uint8_t)(m[i] ? f_in : f_out);
            else ((uint16_t *)dense)[i] = m[i] == s[i] ? ((const uint16_t *)vol)[i] : (uint16_t)(m[i] ? f_in : f_out);
        }
    }
    free(s); free(a); free(m); free(d); free(t0); free(t1);
    return 0;
}
