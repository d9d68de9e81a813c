/* vk_geodesic_distance restated from the rule in include/vokselis_hip.h in plain sequential C: Dijkstra's algorithm with a binary heap
 * over the voxels of S, lazy deletion, the saturating step written as the rule writes it.  No tiles, no rounds, no halos; nothing of the
 * library is included -- the integer square root of a step cost is written out below.  Built with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3 };
#define G_INF 0xFFFFFFFFu
#define G_FAR 0xFFFFFFFEu

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

/* the largest r with r r <= q 65536: counted up from below by halving steps */
static uint32_t step_cost(uint64_t q) {
    const uint64_t target = q * 65536u;
    uint64_t lo = 0, hi = 65536;  /* lo^2 <= target < hi^2: q <= 12288 < 65536 */
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        if (mid * mid <= target) lo = mid; else hi = mid;
    }
    return (uint32_t)lo;
}

typedef struct { uint32_t key, voxel; } entry;
static void heap_push(entry *h, uint64_t *len, entry e) {
    uint64_t i = (*len)++;
    while (i > 0) {
        const uint64_t p = (i - 1) / 2;
        if (h[p].key <= e.key) break;
        h[i] = h[p];
        i = p;
    }
    h[i] = e;
}
static entry heap_pop(entry *h, uint64_t *len) {
    const entry top = h[0], last = h[--(*len)];
    uint64_t i = 0;
    for (;;) {
        uint64_t c = 2 * i + 1;
        if (c >= *len) break;
        if (c + 1 < *len && h[c + 1].key < h[c].key) c++;
        if (h[c].key >= last.key) break;
        h[i] = h[c];
        i = c;
    }
    if (*len) h[i] = last;
    return top;
}

static int on_faces(uint32_t x, uint32_t y, uint32_t z, const uint32_t *box, uint32_t mask) {
    return ((mask & 1u) && x == box[0]) || ((mask & 2u) && x == box[3] - 1u) || ((mask & 4u) && y == box[1]) || ((mask & 8u) && y == box[4] - 1u) ||
           ((mask & 16u) && z == box[2]) || ((mask & 32u) && z == box[5] - 1u);
}

/* vol: nx ny nz texels.  box: 6.  spacing: 3.  seeds: 3 per seed.  g: nx ny nz uint32.  dense: nx ny nz texels.  gain: 0 asks for the
 * automatic one.  result: n_foreground, n_sources, n_reached, n_saturated, n_target_reached, sum_g, max_g, target_min, the bits of the
 * gain used.  Returns 0, or -1 when memory runs out. */
int geo_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, float lo, float hi, uint32_t connectivity, const uint32_t *spacing, uint32_t source_faces,
                uint32_t target_faces, uint32_t n_seeds, const uint32_t *seeds, float gain, float fill_out, float fill_unreached, const uint32_t *box, uint32_t *g, void *dense,
                uint64_t *result) {
    const uint64_t n = (uint64_t)nx * ny * nz;
    const float lo_k = fmt == FMT_U8 ? lo * 255.0f : (fmt == FMT_U16 ? lo * 65535.0f : lo);
    const float hi_k = fmt == FMT_U8 ? hi * 255.0f : (fmt == FMT_U16 ? hi * 65535.0f : hi);
    const int reach = connectivity == 6u ? 1 : (connectivity == 18u ? 2 : 3);
    uint8_t *s = calloc(n ? n : 1, 1), *done = calloc(n ? n : 1, 1);
    entry *heap = malloc((n * 27u + 1u) * sizeof *heap);  /* every push is a lowering over one of at most 26 edges into a voxel, or a source */
    if (!s || !done || !heap) { free(s); free(done); free(heap); return -1; }
    uint64_t len = 0;
    memset(result, 0, 9 * sizeof *result);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = (uint32_t)(i % nx), y = (uint32_t)(i / nx % ny), z = (uint32_t)(i / ((uint64_t)nx * ny));
        const float t = texel(vol, i, fmt);
        s[i] = x >= box[0] && x < box[3] && y >= box[1] && y < box[4] && z >= box[2] && z < box[5] && t >= lo_k && t <= hi_k;
        g[i] = G_INF;
        result[0] += s[i];
        if (!s[i]) continue;
        int source = on_faces(x, y, z, box, source_faces);
        for (uint32_t k = 0; k < n_seeds; k++) source = source || (seeds[3 * k] == x && seeds[3 * k + 1] == y && seeds[3 * k + 2] == z);
        if (source) {
            g[i] = 0u;
            result[1]++;
            heap_push(heap, &len, (entry){0u, (uint32_t)i});
        }
    }
    while (len) {
        const entry e = heap_pop(heap, &len);
        if (done[e.voxel] || e.key != g[e.voxel]) continue;
        done[e.voxel] = 1;
        const int64_t x = e.voxel % nx, y = e.voxel / nx % ny, z = e.voxel / ((uint64_t)nx * ny);
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int steps = abs(dx) + abs(dy) + abs(dz);
                    if (steps < 1 || steps > reach) continue;
                    const int64_t ux = x + dx, uy = y + dy, uz = z + dz;
                    if (ux < 0 || uy < 0 || uz < 0 || ux >= (int64_t)nx || uy >= (int64_t)ny || uz >= (int64_t)nz) continue;
                    const uint64_t iu = (uint64_t)ux + (uint64_t)nx * ((uint64_t)uy + (uint64_t)ny * (uint64_t)uz);
                    if (!s[iu] || done[iu]) continue;
                    const int64_t ex = (int64_t)spacing[0] * dx, ey = (int64_t)spacing[1] * dy, ez = (int64_t)spacing[2] * dz;
                    const uint64_t sum = (uint64_t)e.key + step_cost((uint64_t)(ex * ex + ey * ey + ez * ez));
                    const uint32_t cand = sum < (uint64_t)G_FAR ? (uint32_t)sum : G_FAR;
                    if (cand < g[iu]) {
                        g[iu] = cand;
                        heap_push(heap, &len, (entry){cand, (uint32_t)iu});
                    }
                }
    }
    result[7] = G_INF;
    for (uint64_t i = 0; i < n; i++) {
        if (!s[i] || g[i] == G_INF) continue;
        const uint32_t x = (uint32_t)(i % nx), y = (uint32_t)(i / nx % ny), z = (uint32_t)(i / ((uint64_t)nx * ny));
        result[2]++;
        result[3] += g[i] == G_FAR;
        result[5] += g[i];
        if (g[i] > result[6]) result[6] = g[i];
        if (on_faces(x, y, z, box, target_faces)) {
            result[4]++;
            if (g[i] < result[7]) result[7] = g[i];
        }
    }
    if (gain == 0.0f) gain = result[6] ? 1.0f / (float)(uint32_t)result[6] : 0.0f;
    uint32_t gbits;
    memcpy(&gbits, &gain, 4);
    result[8] = gbits;
    const uint32_t f_out = store_bits(fill_out, fmt), f_un = store_bits(fill_unreached, fmt);
    for (uint64_t i = 0; i < n; i++) {
        uint32_t bits = s[i] ? f_un : f_out;
        if (s[i] && g[i] != G_INF) {
            const float f = (float)g[i];
            const float w = f * gain;
            bits = store_bits(w, fmt);
        }
        if (fmt == FMT_U8) ((uint8_t *)dense)[i] = (uint8_t)bits;
        else ((uint16_t *)dense)[i] = (uint16_t)bits;
    }
    free(s); free(done); free(heap);
    return 0;
}
