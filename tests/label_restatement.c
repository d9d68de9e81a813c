/* vk_label_components restated from the rule in include/vokselis_hip.h in plain sequential C: a raster scan, a flood fill from each
 * unvisited foreground voxel -- ids come out in the order of `first` by construction -- then the selection and the mask.  Shares
 * nothing with the library's union-find.  Built with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3 };
enum { KEEP_ALL = 0, KEEP_LARGEST = 1, KEEP_MIN_SIZE = 2, KEEP_SEEDS = 3 };

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
    (void)frexpf(a, &ex);                 /* a = m 2^ex, 0.5 <= m < 1 */
    int q = ex - 11;                      /* the unit of the half's significand: 11 bits */
    if (q < -24) q = -24;                 /* denormals: the unit stays 2^-24 */
    const float scaled = ldexpf(a, -q);   /* exact: a power of two */
    const float r = rintf(scaled);        /* ties to even (the default rounding mode) */
    const float back = ldexpf(r, q);
    if (back >= 65520.0f) return (uint16_t)(sign | 0x7c00u);
    if (back < 6.103515625e-05f) return (uint16_t)(sign | (uint16_t)r);  /* below 2^-14: r units of 2^-24 */
    int e2;
    const float m2 = frexpf(back, &e2);   /* back = m2 2^e2 */
    return (uint16_t)(sign | (uint16_t)(((e2 + 14) << 10) | ((uint32_t)ldexpf(m2, 11) & 1023u)));
}

static float texel(const void *vol, uint64_t i, int fmt) {
    if (fmt == FMT_U8) return (float)((const uint8_t *)vol)[i];
    if (fmt == FMT_U16) return (float)((const uint16_t *)vol)[i];
    return half_value(((const uint16_t *)vol)[i]);
}

/* labels: nx ny nz uint32.  table: cap x 8 uint64 (n_voxels, first, x0, y0, z0, x1, y1, z1), may be NULL.  result: 4 uint64.  dense:
 * nx ny nz texels, may be NULL.  seeds: n_seeds x 3.  box: 6.  Returns 0, or -1 when memory runs out. */
int label_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, float lo, float hi, uint32_t connectivity, const uint32_t *box, int keep, uint64_t count,
                  uint32_t n_seeds, const uint32_t *seeds, int invert, float fill, uint32_t *labels, uint64_t *table, uint64_t cap, uint64_t *result, void *dense) {
    const uint64_t n = (uint64_t)nx * ny * nz;
    const float scale = fmt == FMT_U8 ? 255.0f : (fmt == FMT_U16 ? 65535.0f : 1.0f);
    const float lo_k = fmt == FMT_F16 ? lo : lo * scale, hi_k = fmt == FMT_F16 ? hi : hi * scale;
    const int most = connectivity == 6u ? 1 : (connectivity == 18u ? 2 : 3);
    uint8_t *fg = malloc(n ? n : 1);
    uint32_t *stack = malloc((n ? n : 1) * sizeof *stack);
    uint64_t *rec = NULL;  /* 8 per component, grown as they are found */
    uint64_t n_comp = 0, rec_cap = 0, n_fg = 0;
    if (!fg || !stack) { free(fg); free(stack); return -1; }
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = (uint32_t)(i % nx), y = (uint32_t)(i / nx % ny), z = (uint32_t)(i / ((uint64_t)nx * ny));
        const float t = texel(vol, i, fmt);
        fg[i] = x >= box[0] && x < box[3] && y >= box[1] && y < box[4] && z >= box[2] && z < box[5] && t >= lo_k && t <= hi_k;
        labels[i] = 0;
    }
    for (uint64_t s = 0; s < n; s++) {
        if (!fg[s] || labels[s]) continue;
        if (n_comp == rec_cap) {
            rec_cap = rec_cap ? 2 * rec_cap : 64;
            uint64_t *grown = realloc(rec, rec_cap * 8 * sizeof *rec);
            if (!grown) { free(fg); free(stack); free(rec); return -1; }
            rec = grown;
        }
        uint64_t *r = rec + 8 * n_comp;
        const uint32_t id = (uint32_t)++n_comp;
        r[0] = 0; r[1] = s;
        r[2] = r[3] = r[4] = UINT64_MAX; r[5] = r[6] = r[7] = 0;
        uint64_t top = 0;
        stack[top++] = (uint32_t)s;
        labels[s] = id;
        while (top) {
            const uint64_t i = stack[--top];
            const int64_t c[3] = {(int64_t)(i % nx), (int64_t)(i / nx % ny), (int64_t)(i / ((uint64_t)nx * ny))};
            r[0]++; n_fg++;
            for (int a = 0; a < 3; a++) {
                if ((uint64_t)c[a] < r[2 + a]) r[2 + a] = (uint64_t)c[a];
                if ((uint64_t)c[a] + 1 > r[5 + a]) r[5 + a] = (uint64_t)c[a] + 1;
            }
            for (int dz = -1; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int sum = abs(dx) + abs(dy) + abs(dz);
                        const int64_t x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
                        if (sum < 1 || sum > most || x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) continue;
                        const uint64_t j = (uint64_t)x + (uint64_t)nx * ((uint64_t)y + (uint64_t)ny * (uint64_t)z);
                        if (fg[j] && !labels[j]) { labels[j] = id; stack[top++] = (uint32_t)j; }
                    }
        }
    }
    /* the selection */
    uint8_t *sel = calloc(n_comp + 1, 1);
    if (!sel) { free(fg); free(stack); free(rec); return -1; }
    if (keep == KEEP_ALL) memset(sel + 1, 1, n_comp);
    else if (keep == KEEP_MIN_SIZE) { for (uint64_t k = 0; k < n_comp; k++) sel[k + 1] = rec[8 * k] >= count; }
    else if (keep == KEEP_SEEDS) {
        for (uint32_t s = 0; s < n_seeds; s++) {
            const uint32_t id = labels[seeds[3 * s] + (uint64_t)nx * (seeds[3 * s + 1] + (uint64_t)ny * seeds[3 * s + 2])];
            if (id) sel[id] = 1;
        }
    } else {
        for (uint64_t round = 0; round < count && round < n_comp; round++) {  /* the largest not yet taken; of equals the one with the smallest first */
            uint64_t best = UINT64_MAX;
            for (uint64_t k = 0; k < n_comp; k++)
                if (!sel[k + 1] && (best == UINT64_MAX || rec[8 * k] > rec[8 * best])) best = k;
            sel[best + 1] = 1;
        }
    }
    result[0] = n_comp; result[1] = n_fg; result[2] = 0; result[3] = 0;
    for (uint64_t k = 0; k < n_comp; k++)
        if (sel[k + 1]) { result[2]++; result[3] += rec[8 * k]; }
    if (table) memcpy(table, rec, (n_comp < cap ? n_comp : cap) * 8 * sizeof *rec);
    if (dense) {
        uint32_t F;
        if (fmt == FMT_F16) F = half_bits(fill);
        else F = (uint32_t)rintf(fminf(fmaxf(fill * scale, 0.0f), scale));
        for (uint64_t i = 0; i < n; i++) {
            const int m = sel[labels[i]];
            const int stays = invert ? !m : m;
            if (fmt == FMT_U8) ((uint8_t *)dense)[i] = stays ? ((const uint8_t *)vol)[i] : (uint8_t)F;
            else ((uint16_t *)dense)[i] = stays ? ((const uint16_t *)vol)[i] : (uint16_t)F;
        }
    }
    free(fg); free(stack); free(rec); free(sel);
    return 0;
}
