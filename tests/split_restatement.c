/* vk_split_components restated from the rule in include/vokselis_hip.h in plain sequential C: the squared distance to the complement by
 * three nested minima over whole lines, a flood fill of the eroded set in raster order (anchors), a breadth-first growth by rounds in
 * which a round only looks at what the round before labelled, a flood fill of what no marker reached, the numbering by increasing anchor,
 * the table and the cut.  Shares nothing with the library's union-find, envelopes or double-buffered rounds.  Built with
 * -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3 };
#define NONE UINT64_MAX
#define NO_G 0xffffffffu

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

/* along one axis: out(i) = min over j of in(j) + (w (i - j))^2, NONE where every in(j) is NONE */
static void axis_minimum(const uint64_t *in, uint64_t *out, uint64_t base, uint64_t stride, uint32_t n, uint64_t w) {
    for (uint32_t i = 0; i < n; i++) {
        uint64_t best = NONE;
        for (uint32_t j = 0; j < n; j++) {
            const uint64_t g = in[base + j * stride];
            if (g == NONE) continue;
            const uint64_t d = w * (uint64_t)(i > j ? i - j : j - i), v = g + d * d;
            if (v < best) best = v;
        }
        out[base + i * stride] = best;
    }
}

typedef struct { uint32_t nx, ny, nz; int most; } grid;

/* the neighbours of voxel i under the connectivity, into out (at most 26); returns how many */
static int neighbours(const grid *G, uint64_t i, uint64_t *out) {
    const int64_t cx = (int64_t)(i % G->nx), cy = (int64_t)(i / G->nx % G->ny), cz = (int64_t)(i / ((uint64_t)G->nx * G->ny));
    int k = 0;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int sum = abs(dx) + abs(dy) + abs(dz);
                const int64_t x = cx + dx, y = cy + dy, z = cz + dz;
                if (sum < 1 || sum > G->most || x < 0 || y < 0 || z < 0 || x >= G->nx || y >= G->ny || z >= G->nz) continue;
                out[k++] = (uint64_t)x + (uint64_t)G->nx * ((uint64_t)y + (uint64_t)G->ny * (uint64_t)z);
            }
    return k;
}

/* every voxel of `in` that has no anchor yet takes the smallest index of its component within `in` (raster order: the start of a fill) */
static void fill_anchors(const grid *G, const uint8_t *in, uint64_t n, uint64_t *anchor, uint64_t *stack, uint64_t *n_comp, uint64_t *n_vox) {
    uint64_t nb[26];
    for (uint64_t s = 0; s < n; s++) {
        if (!in[s] || anchor[s] != NONE) continue;
        (*n_comp)++;
        uint64_t top = 0;
        stack[top++] = s;
        anchor[s] = s;
        while (top) {
            const uint64_t i = stack[--top];
            (*n_vox)++;
            const int k = neighbours(G, i, nb);
            for (int a = 0; a < k; a++)
                if (in[nb[a]] && anchor[nb[a]] == NONE) { anchor[nb[a]] = s; stack[top++] = nb[a]; }
        }
    }
}

/* labels: nx ny nz uint32.  table: cap x 8 uint64 (n_voxels, anchor, x0, y0, z0, x1, y1, z1), may be NULL.  result: 8 uint64 (n_regions,
 * n_foreground, n_markers, n_marker_voxels, n_residue_regions, n_residue_voxels, n_cut, rounds).  dense: nx ny nz texels, may be NULL.
 * g_out: nx ny nz uint32, may be NULL: g, 0xffffffff where it is not finite.  box: 6.  spacing: 3.  Returns 0, or -1 when memory runs out. */
int split_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, float lo, float hi, uint32_t connectivity, const uint32_t *box, const uint32_t *spacing, float radius,
                  float fill_out, uint32_t *labels, uint64_t *table, uint64_t cap, uint64_t *result, void *dense, uint32_t *g_out) {
    const uint64_t n = (uint64_t)nx * ny * nz, room = n ? n : 1;
    const float scale = fmt == FMT_U8 ? 255.0f : (fmt == FMT_U16 ? 65535.0f : 1.0f);
    const float lo_k = fmt == FMT_F16 ? lo : lo * scale, hi_k = fmt == FMT_F16 ? hi : hi * scale;
    const grid G = {nx, ny, nz, connectivity == 6u ? 1 : (connectivity == 18u ? 2 : 3)};
    const uint64_t r2 = (uint64_t)floor((double)radius * (double)radius);
    uint8_t *fg = calloc(room, 1), *K = calloc(room, 1);
    uint64_t *d_a = malloc(room * 8), *d_b = malloc(room * 8), *anchor = malloc(room * 8), *list = malloc(room * 8), *next = malloc(room * 8), *rec = NULL;
    uint32_t *g = malloc(room * 4);
    int rc = -1;
    if (!fg || !K || !d_a || !d_b || !anchor || !list || !next || !g) goto done;

    uint64_t n_fg = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = (uint32_t)(i % nx), y = (uint32_t)(i / nx % ny), z = (uint32_t)(i / ((uint64_t)nx * ny));
        const float t = texel(vol, i, fmt);
        fg[i] = x >= box[0] && x < box[3] && y >= box[1] && y < box[4] && z >= box[2] && z < box[5] && t >= lo_k && t <= hi_k;
        n_fg += fg[i];
        d_a[i] = fg[i] ? NONE : 0;  /* the distance to not S starts at 0 on not S */
        labels[i] = 0;
        anchor[i] = NONE;
        g[i] = NO_G;
    }
    /* D2(not S, .): min over x', then y', then z' */
    for (uint64_t line = 0; line < (uint64_t)ny * nz; line++) axis_minimum(d_a, d_b, line * nx, 1, nx, spacing[0]);
    for (uint32_t z = 0; z < nz; z++)
        for (uint32_t x = 0; x < nx; x++) axis_minimum(d_b, d_a, x + (uint64_t)nx * ny * z, nx, ny, spacing[1]);
    for (uint64_t col = 0; col < (uint64_t)nx * ny; col++) axis_minimum(d_a, d_b, col, (uint64_t)nx * ny, nz, spacing[2]);
    for (uint64_t i = 0; i < n; i++) K[i] = fg[i] && d_b[i] > r2;  /* NONE: no voxel outside S at all, and VK_DIST_INF > R2 */

    /* the markers and their anchors */
    uint64_t n_markers = 0, n_marker_voxels = 0;
    fill_anchors(&G, K, n, anchor, list, &n_markers, &n_marker_voxels);

    /* the growth: round k looks at the voxels round k - 1 labelled (g == k - 1), and at nothing round k itself writes */
    uint64_t n_list = 0, nb[26];
    uint32_t rounds = 0;
    for (uint64_t i = 0; i < n; i++)
        if (K[i]) { g[i] = 0; list[n_list++] = i; }
    for (uint32_t k = 1; n_list; k++) {
        uint64_t n_next = 0;
        for (uint64_t q = 0; q < n_list; q++) {
            const uint64_t u = list[q];
            const int m = neighbours(&G, u, nb);
            for (int a = 0; a < m; a++) {
                const uint64_t v = nb[a];
                if (!fg[v] || g[v] < k) continue;               /* off S, or labelled in an earlier round */
                if (g[v] == NO_G) { g[v] = k; anchor[v] = anchor[u]; next[n_next++] = v; }
                else if (anchor[u] < anchor[v]) anchor[v] = anchor[u];  /* g[v] == k: another neighbour of round k - 1 */
            }
        }
        if (n_next) rounds = k;
        uint64_t *t = list; list = next; next = t;
        n_list = n_next;
    }

    /* what no marker reached: components of its own */
    uint64_t n_res = 0, n_res_voxels = 0;
    for (uint64_t i = 0; i < n; i++) K[i] = fg[i] && anchor[i] == NONE;
    fill_anchors(&G, K, n, anchor, list, &n_res, &n_res_voxels);

    /* regions by increasing anchor: an anchor is a voxel that is its own anchor, met in raster order */
    const uint64_t n_reg = n_markers + n_res;
    rec = malloc((n_reg ? n_reg : 1) * 8 * sizeof *rec);
    if (!rec) goto done;
    uint64_t id = 0;
    for (uint64_t i = 0; i < n; i++)
        if (fg[i] && anchor[i] == i) {
            uint64_t *r = rec + 8 * id;
            r[0] = 0; r[1] = i; r[2] = r[3] = r[4] = UINT64_MAX; r[5] = r[6] = r[7] = 0;
            labels[i] = (uint32_t)++id;
        }
    if (id != n_reg) { rc = -2; goto done; }
    for (uint64_t i = 0; i < n; i++) {
        if (!fg[i]) continue;
        labels[i] = labels[anchor[i]];
        uint64_t *r = rec + 8 * (uint64_t)(labels[i] - 1);
        const uint64_t c[3] = {i % nx, i / nx % ny, i / ((uint64_t)nx * ny)};
        r[0]++;
        for (int a = 0; a < 3; a++) {
            if (c[a] < r[2 + a]) r[2 + a] = c[a];
            if (c[a] + 1 > r[5 + a]) r[5 + a] = c[a] + 1;
        }
    }
    /* the cut */
    uint32_t F;
    if (fmt == FMT_F16) F = half_bits(fill_out);
    else F = (uint32_t)rintf(fminf(fmaxf(fill_out * scale, 0.0f), scale));
    uint64_t n_cut = 0;
    for (uint64_t i = 0; i < n; i++) {
        int cut = 0;
        if (fg[i]) {
            const int m = neighbours(&G, i, nb);
            for (int a = 0; a < m; a++) cut = cut || (fg[nb[a]] && labels[nb[a]] < labels[i]);
        }
        n_cut += (uint64_t)cut;
        if (!dense) continue;
        if (fmt == FMT_U8) ((uint8_t *)dense)[i] = cut ? (uint8_t)F : ((const uint8_t *)vol)[i];
        else ((uint16_t *)dense)[i] = cut ? (uint16_t)F : ((const uint16_t *)vol)[i];
    }
    if (table) memcpy(table, rec, (n_reg < cap ? n_reg : cap) * 8 * sizeof *rec);
    if (g_out) memcpy(g_out, g, n * 4);
    result[0] = n_reg; result[1] = n_fg; result[2] = n_markers; result[3] = n_marker_voxels; result[4] = n_res; result[5] = n_res_voxels; result[6] = n_cut; result[7] = rounds;
    rc = 0;
done:
    free(fg); free(K); free(d_a); free(d_b); free(anchor); free(list); free(next); free(g); free(rec);
    return rc;
}
