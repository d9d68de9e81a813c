/* vk_skeletonize restated from the rule in include/vokselis_hip.h in plain sequential C: per sub-pass the deletable voxels are collected
 * in raster order and then deleted.  The simple-point test copies a voxel's neighbourhood into an explicit 3 x 3 x 3 array and flood
 * fills it with a stack.  No tiles, no halos, no state bytes, no bit masks; nothing of the library is included.  Built with
 * -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { FMT_U8 = 0, FMT_F16 = 1, FMT_U16 = 3 };
enum { MODE_CURVE = 0, MODE_KERNEL = 1 };
enum { R_FOREGROUND = 0, R_SKELETON = 1, R_CLASS = 1 /* + class 1 .. 4 */, R_LINKS = 6, R_ITERATIONS = 19, R_CONVERGED = 20, R_WORDS = 21 };

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

typedef struct { uint32_t nx, ny, nz; const uint8_t *k; } grid;
static int in_set(const grid *g, int64_t x, int64_t y, int64_t z) {
    if (x < 0 || y < 0 || z < 0 || x >= (int64_t)g->nx || y >= (int64_t)g->ny || z >= (int64_t)g->nz) return 0;
    return g->k[(uint64_t)x + (uint64_t)g->nx * ((uint64_t)y + (uint64_t)g->ny * (uint64_t)z)];
}

/* the neighbourhood of (x, y, z) as nb[dz + 1][dy + 1][dx + 1]; the centre is left 0.  Returns how many neighbours are in the set. */
static int neighbourhood(const grid *g, int64_t x, int64_t y, int64_t z, int nb[3][3][3]) {
    int count = 0;
    for (int dz = -1; dz <= 1; dz++)
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int v = (dx || dy || dz) ? in_set(g, x + dx, y + dy, z + dz) : 0;
                nb[dz + 1][dy + 1][dx + 1] = v;
                count += v;
            }
    return count;
}

/* Flood fill over the cells with allowed[..] != 0 and seen[..] == 0 from (z, y, x): steps of at most `reach` axes at once (3: the 26
 * neighbours, 1: the 6), never onto the centre. */
static void flood(int allowed[3][3][3], int seen[3][3][3], int z, int y, int x, int reach) {
    int stack[27][3], top = 0;
    seen[z][y][x] = 1;
    stack[top][0] = z; stack[top][1] = y; stack[top][2] = x; top++;
    while (top) {
        top--;
        const int cz = stack[top][0], cy = stack[top][1], cx = stack[top][2];
        for (int dz = -1; dz <= 1; dz++)
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int steps = abs(dx) + abs(dy) + abs(dz);
                    const int uz = cz + dz, uy = cy + dy, ux = cx + dx;
                    if (steps < 1 || steps > reach || uz < 0 || uy < 0 || ux < 0 || uz > 2 || uy > 2 || ux > 2) continue;
                    if (uz == 1 && uy == 1 && ux == 1) continue;
                    if (!allowed[uz][uy][ux] || seen[uz][uy][ux]) continue;
                    seen[uz][uy][ux] = 1;
                    stack[top][0] = uz; stack[top][1] = uy; stack[top][2] = ux; top++;
                }
    }
}

static int simple_point(int nb[3][3][3]) {
    /* (a) the set cells among the 26: exactly one 26-component */
    int seen[3][3][3] = {{{0}}}, components = 0;
    for (int z = 0; z < 3; z++)
        for (int y = 0; y < 3; y++)
            for (int x = 0; x < 3; x++) {
                if ((z == 1 && y == 1 && x == 1) || !nb[z][y][x] || seen[z][y][x]) continue;
                components++;
                flood(nb, seen, z, y, x, 3);
            }
    if (components != 1) return 0;
    /* (b) the clear cells among the 18 with |d|_1 <= 2: exactly one 6-component that holds a face cell */
    int open[3][3][3];
    for (int z = 0; z < 3; z++)
        for (int y = 0; y < 3; y++)
            for (int x = 0; x < 3; x++) {
                const int d1 = abs(z - 1) + abs(y - 1) + abs(x - 1);
                open[z][y][x] = d1 >= 1 && d1 <= 2 && !nb[z][y][x];
            }
    memset(seen, 0, sizeof seen);
    components = 0;
    static const int face[6][3] = {{0, 1, 1}, {2, 1, 1}, {1, 0, 1}, {1, 2, 1}, {1, 1, 0}, {1, 1, 2}};
    for (int f = 0; f < 6; f++) {
        const int z = face[f][0], y = face[f][1], x = face[f][2];
        if (!open[z][y][x] || seen[z][y][x]) continue;
        components++;
        flood(open, seen, z, y, x, 1);
    }
    return components == 1;
}

/* vol: nx ny nz texels, x fastest.  box: x0 y0 z0 x1 y1 z1.  classes: nx ny nz bytes; dense: nx ny nz texels; result: R_WORDS words. */
int skel_restate(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, float lo, float hi, int mode, uint32_t max_iterations, int fill_in_on, float fill_in, float fill_out,
                 const uint32_t *box, uint8_t *classes, void *dense, uint64_t *result) {
    const uint64_t n = (uint64_t)nx * ny * nz;
    const float lo_k = fmt == FMT_U8 ? lo * 255.0f : (fmt == FMT_U16 ? lo * 65535.0f : lo);
    const float hi_k = fmt == FMT_U8 ? hi * 255.0f : (fmt == FMT_U16 ? hi * 65535.0f : hi);
    uint8_t *k = calloc(n ? n : 1, 1), *start = calloc(n ? n : 1, 1);
    uint64_t *doomed = malloc((n ? n : 1) * sizeof *doomed);
    if (!k || !start || !doomed) { free(k); free(start); free(doomed); return -1; }
    memset(result, 0, R_WORDS * sizeof *result);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t x = (uint32_t)(i % nx), y = (uint32_t)(i / nx % ny), z = (uint32_t)(i / ((uint64_t)nx * ny));
        const float t = texel(vol, i, fmt);
        k[i] = x >= box[0] && x < box[3] && y >= box[1] && y < box[4] && z >= box[2] && z < box[5] && t >= lo_k && t <= hi_k;
        result[R_FOREGROUND] += k[i];
    }
    const grid now = {nx, ny, nz, k}, then = {nx, ny, nz, start};
    for (uint32_t iteration = 1; max_iterations == 0u || iteration <= max_iterations; iteration++) {
        memcpy(start, k, n);  /* K_i */
        uint64_t deleted = 0;
        for (uint32_t s = 0; s < 8u; s++) {
            uint64_t count = 0;
            for (uint64_t i = 0; i < n; i++) {
                const int64_t x = (int64_t)(i % nx), y = (int64_t)(i / nx % ny), z = (int64_t)(i / ((uint64_t)nx * ny));
                if (!k[i] || (uint32_t)((x & 1) | ((y & 1) << 1) | ((z & 1) << 2)) != s) continue;
                /* a candidate: in K_i (it is: nothing joins K) with a face neighbour that is not */
                if (in_set(&then, x - 1, y, z) && in_set(&then, x + 1, y, z) && in_set(&then, x, y - 1, z) && in_set(&then, x, y + 1, z) && in_set(&then, x, y, z - 1) &&
                    in_set(&then, x, y, z + 1))
                    continue;
                int nb[3][3][3];
                const int neighbours = neighbourhood(&now, x, y, z, nb);
                if (mode == MODE_CURVE && neighbours == 1) continue;
                if (simple_point(nb)) doomed[count++] = i;
            }
            for (uint64_t j = 0; j < count; j++) k[doomed[j]] = 0;
            deleted += count;
        }
        if (!deleted) { result[R_CONVERGED] = 1; break; }
        result[R_ITERATIONS]++;
    }
    const uint32_t f_in = store_bits(fill_in_on ? fill_in : 0.0f, fmt), f_out = store_bits(fill_out, fmt);
    for (uint64_t i = 0; i < n; i++) {
        const int64_t x = (int64_t)(i % nx), y = (int64_t)(i / nx % ny), z = (int64_t)(i / ((uint64_t)nx * ny));
        uint32_t bits = f_out;
        classes[i] = 0;
        if (k[i]) {
            int nb[3][3][3];
            const int neighbours = neighbourhood(&now, x, y, z, nb);
            const int c = neighbours >= 3 ? 4 : 1 + neighbours;
            classes[i] = (uint8_t)c;
            result[R_SKELETON]++;
            result[R_CLASS + c]++;
            /* the offsets above the centre in the order dz, dy, dx: each unordered pair once, from its earlier end */
            int j = 0;
            for (int dz = 0; dz <= 1; dz++)
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        if (dz == 0 && (dy < 0 || (dy == 0 && dx <= 0))) continue;
                        result[R_LINKS + j] += (uint64_t)nb[dz + 1][dy + 1][dx + 1];
                        j++;
                    }
            bits = fill_in_on ? f_in : (fmt == FMT_U8 ? ((const uint8_t *)vol)[i] : ((const uint16_t *)vol)[i]);
        }
        if (fmt == FMT_U8) ((uint8_t *)dense)[i] = (uint8_t)bits;
        else ((uint16_t *)dense)[i] = (uint16_t)bits;
    }
    free(k); free(start); free(doomed);
    return 0;
}
