/* vk_steady_diffusion restated from the rule in include/vokselis_hip.h in plain sequential C: a byte per voxel for S, a float per voxel
 * for c, raster loops over the voxels of one colour, then of the other.  No tiles, no rounds, no marker values; nothing of the library is
 * included.  omega is taken as given (the automatic formula is the caller's).  Built with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3 };

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

static int64_t quantise(float t) {
    float k = t;
    if (!(t >= -1048576.0f)) k = -1048576.0f;
    else if (t > 1048576.0f) k = 1048576.0f;
    const float scaled = k * 1073741824.0f;
    return (int64_t)scaled;
}

/* vol: nx ny nz texels.  box: 6.  spacing: 3.  c: nx ny nz floats (the bits 0x7FC00000 off S).  dense: nx ny nz texels.  omega: in (0, 2).
 * gain: 0 asks for 1.  result: n_foreground, n_inlet, n_outlet, n_box, Fin_q, Fout_q, sum_c_q, sweeps, converged, and the bits of delta,
 * of omega and of the gain used.  Returns 0, or -1 when memory runs out. */
int diff_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, float lo, float hi, uint32_t axis, const uint32_t *spacing, float omega, uint32_t check_every,
                 uint32_t max_sweeps, float delta_tol, float flux_tol, float gain, float fill_out, const uint32_t *box, float *c, void *dense, uint64_t *result) {
    const uint64_t n = (uint64_t)nx * ny * nz;
    const float lo_k = fmt == FMT_U8 ? lo * 255.0f : (fmt == FMT_U16 ? lo * 65535.0f : lo);
    const float hi_k = fmt == FMT_U8 ? hi * 255.0f : (fmt == FMT_U16 ? hi * 65535.0f : hi);
    uint8_t *s = calloc(n ? n : 1, 1);
    if (!s) return -1;
    float w[3];
    for (int k = 0; k < 3; k++) w[k] = (float)(1.0 / (double)(spacing[k] * spacing[k]));
    const float g = 2.0f * w[axis];
    const uint32_t first = box[axis], last = box[3 + axis] - 1u;
    memset(result, 0, 12 * sizeof *result);
    result[3] = (uint64_t)(box[3] - box[0]) * (box[4] - box[1]) * (box[5] - box[2]);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t p[3] = {(uint32_t)(i % nx), (uint32_t)(i / nx % ny), (uint32_t)(i / ((uint64_t)nx * ny))};
        const float t = texel(vol, i, fmt);
        s[i] = p[0] >= box[0] && p[0] < box[3] && p[1] >= box[1] && p[1] < box[4] && p[2] >= box[2] && p[2] < box[5] && t >= lo_k && t <= hi_k;
        c[i] = 0.5f;
        result[0] += s[i];
        result[1] += s[i] && p[axis] == first;
        result[2] += s[i] && p[axis] == last;
    }
    const int64_t stride[3] = {1, (int64_t)nx, (int64_t)nx * ny};
    const uint32_t dims[3] = {nx, ny, nz};
    uint32_t blocks = 0, converged = 0;
    float delta = 0.0f;
    int64_t fin = 0, fout = 0;
    while (blocks < max_sweeps / check_every && !converged) {
        for (uint32_t sweep = 0; sweep < check_every; sweep++) {
            if (sweep + 1u == check_every) delta = 0.0f;
            for (uint32_t colour = 0; colour < 2u; colour++)
                for (uint32_t z = 0; z < nz; z++)
                    for (uint32_t y = 0; y < ny; y++)
                        for (uint32_t x = 0; x < nx; x++) {
                            if (((x + y + z) & 1u) != colour) continue;
                            const uint64_t i = (uint64_t)x + (uint64_t)nx * ((uint64_t)y + (uint64_t)ny * z);
                            if (!s[i]) continue;
                            const uint32_t p[3] = {x, y, z};
                            float num = 0.0f, den = 0.0f;
                            for (int k = 0; k < 3; k++)
                                for (int side = -1; side <= 1; side += 2) {
                                    if (side < 0 ? p[k] == 0u : p[k] + 1u == dims[k]) continue;
                                    const uint64_t u = (uint64_t)((int64_t)i + side * stride[k]);
                                    if (!s[u]) continue;
                                    const float term = w[k] * c[u];
                                    num = num + term;
                                    den = den + w[k];
                                }
                            if (p[axis] == first) { num = num + g; den = den + g; }
                            if (p[axis] == last) den = den + g;
                            if (den == 0.0f) continue;
                            const float gs = num / den;
                            const float d = gs - c[i];
                            const float step = omega * d;
                            const float next = c[i] + step;
                            if (sweep + 1u == check_every) {
                                const float moved = fabsf(next - c[i]);
                                if (moved > delta) delta = moved;
                            }
                            c[i] = next;
                        }
        }
        blocks++;
        fin = 0; fout = 0;
        for (uint64_t i = 0; i < n; i++) {
            if (!s[i]) continue;
            const uint32_t p[3] = {(uint32_t)(i % nx), (uint32_t)(i / nx % ny), (uint32_t)(i / ((uint64_t)nx * ny))};
            if (p[axis] == first) fin += quantise(2.0f * (1.0f - c[i]));
            if (p[axis] == last) fout += quantise(2.0f * c[i]);
        }
        const double gap = fabs((double)fin - (double)fout);
        converged = (double)delta <= (double)delta_tol && gap <= (double)flux_tol * 0.5 * ((double)fin + (double)fout);
    }
    int64_t sum_c = 0;
    for (uint64_t i = 0; i < n; i++)
        if (s[i]) sum_c += quantise(c[i]);
    if (gain == 0.0f) gain = 1.0f;
    uint32_t bits;
    result[4] = (uint64_t)fin; result[5] = (uint64_t)fout; result[6] = (uint64_t)sum_c;
    result[7] = (uint64_t)blocks * check_every; result[8] = converged;
    memcpy(&bits, &delta, 4); result[9] = bits;
    memcpy(&bits, &omega, 4); result[10] = bits;
    memcpy(&bits, &gain, 4); result[11] = bits;
    const uint32_t f_out = store_bits(fill_out, fmt), off = 0x7FC00000u;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t out = f_out;
        if (s[i]) {
            const float v = c[i] * gain;
            out = store_bits(v, fmt);
        } else memcpy(&c[i], &off, 4);
        if (fmt == FMT_U8) ((uint8_t *)dense)[i] = (uint8_t)out;
        else ((uint16_t *)dense)[i] = (uint16_t)out;
    }
    free(s);
    return 0;
}
