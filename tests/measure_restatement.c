/* vk_measure_components restated from the rule in include/vokselis_hip.h, voxel by voxel: one walk over the volume
 * in raster order, every sum in __int128, every neighbour looked up by its coordinates.  It knows nothing of runs, limbs, chunks or
 * tables, and shares no code with the library or with tests/np_measure_reference.py.  The labels are an input: the tests take them from
 * the label restatement (source "range") or from the case (source "labels").
 *
 * out: n_regions rows of 27 uint64 --
 *   0 n_voxels  1 first  2..7 box (x0 y0 z0 x1 y1 z1, zeros when empty)  8..16 sums (x y z xx yy zz xy xz yz)  17 n_nonfinite
 *   18 q_min  19 q_max (two's complement)  20 sum_q_hi  21 sum_q_lo  22 sum_qq_hi  23 sum_qq_lo  24..26 faces (x y z) */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3, COLS = 27 };

typedef struct {
    unsigned __int128 n, sums[9], qq, nonfinite, faces[3];
    __int128 q;
    uint64_t first, lo[3], hi[3];
    int64_t q_min, q_max;
} region;

/* the texel on the integer scale: the stored integer, or the half's value times 2^24 (exact in double) */
static int texel_q(const void *vol, int format, uint64_t i, int64_t *q) {
    if (format == FMT_U8) { *q = ((const uint8_t *)vol)[i]; return 1; }
    if (format == FMT_U16) { *q = ((const uint16_t *)vol)[i]; return 1; }
    const uint16_t h = ((const uint16_t *)vol)[i];
    const int e = (h >> 10) & 31, m = h & 1023;
    if (e == 31) { *q = 0; return 0; }
    double v = e == 0 ? ldexp((double)m, -24) : ldexp((double)(m + 1024), e - 25);
    if (h & 0x8000) v = -v;
    *q = (int64_t)ldexp(v, 24);
    return 1;
}

static uint32_t label_at(const uint32_t *labels, int64_t x, int64_t y, int64_t z, int64_t nx, int64_t ny, int64_t nz) {
    if (x < 0 || y < 0 || z < 0 || x >= nx || y >= ny || z >= nz) return 0u;
    return labels[x + nx * (y + ny * z)];
}

/* 0, or 2 when a label exceeds n_regions (the library refuses such an array) */
int measure_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, const uint32_t *labels, uint64_t n_regions, uint64_t *out, uint64_t *n_foreground) {
    region *r = (region *)calloc(n_regions ? n_regions : 1, sizeof(region));
    if (!r) return 1;
    for (uint64_t k = 0; k < n_regions; k++) {
        r[k].first = UINT64_MAX;
        r[k].q_min = INT64_MAX;
        r[k].q_max = INT64_MIN;
        for (int a = 0; a < 3; a++) r[k].lo[a] = UINT64_MAX;
    }
    uint64_t fg = 0;
    for (uint32_t z = 0; z < nz; z++)
        for (uint32_t y = 0; y < ny; y++)
            for (uint32_t x = 0; x < nx; x++) {
                const uint64_t i = x + (uint64_t)nx * (y + (uint64_t)ny * z);
                const uint32_t id = labels[i];
                if (id == 0u) continue;
                if (id > n_regions) { free(r); return 2; }
                fg++;
                region *g = r + (id - 1u);
                const uint64_t c[3] = {x, y, z};
                g->n++;
                if (i < g->first) g->first = i;
                for (int a = 0; a < 3; a++) {
                    if (c[a] < g->lo[a]) g->lo[a] = c[a];
                    if (c[a] + 1u > g->hi[a]) g->hi[a] = c[a] + 1u;
                    g->sums[a] += c[a];
                    g->sums[3 + a] += (unsigned __int128)c[a] * c[a];
                }
                g->sums[6] += (unsigned __int128)x * y;
                g->sums[7] += (unsigned __int128)x * z;
                g->sums[8] += (unsigned __int128)y * z;
                int64_t q;
                if (texel_q(vol, format, i, &q)) {
                    if (q < g->q_min) g->q_min = q;
                    if (q > g->q_max) g->q_max = q;
                    g->q += q;
                    g->qq += (unsigned __int128)((__int128)q * q);
                } else g->nonfinite++;
                for (int a = 0; a < 3; a++)
                    for (int s = -1; s <= 1; s += 2) {
                        const int64_t hx = (int64_t)x + (a == 0 ? s : 0), hy = (int64_t)y + (a == 1 ? s : 0), hz = (int64_t)z + (a == 2 ? s : 0);
                        if (label_at(labels, hx, hy, hz, nx, ny, nz) != id) g->faces[a]++;
                    }
            }
    for (uint64_t k = 0; k < n_regions; k++) {
        uint64_t *o = out + k * COLS;
        const region *g = r + k;
        memset(o, 0, COLS * sizeof(uint64_t));
        o[0] = (uint64_t)g->n;
        o[1] = g->first;
        if (g->n)
            for (int a = 0; a < 3; a++) { o[2 + a] = g->lo[a]; o[5 + a] = g->hi[a]; }
        for (int a = 0; a < 9; a++) {
            if (g->sums[a] >> 64) { free(r); return 3; }  /* the library refuses a volume where this can happen */
            o[8 + a] = (uint64_t)g->sums[a];
        }
        o[17] = (uint64_t)g->nonfinite;
        o[18] = (uint64_t)g->q_min;
        o[19] = (uint64_t)g->q_max;
        o[20] = (uint64_t)(g->q >> 64);
        o[21] = (uint64_t)g->q;
        o[22] = (uint64_t)(g->qq >> 64);
        o[23] = (uint64_t)g->qq;
        for (int a = 0; a < 3; a++) o[24 + a] = (uint64_t)g->faces[a];
    }
    *n_foreground = fg;
    free(r);
    return 0;
}
