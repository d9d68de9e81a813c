/* The rule of vk_extract_isosurface restated over the dense array: marching tetrahedra on the 6-tetrahedra split of
 * every cube of a voxel box, operation by operation in f32.  Compiled with -ffp-contract=off; includes none of the library's headers and
 * carries its own half conversion.  The tests hold it to an independent numpy statement (tests/np_mesh_reference.py) and the kernels to it. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h >> 15) << 31, exp = (h >> 10) & 31u, man = h & 1023u;
    uint32_t bits;
    float f;
    if (exp == 31u) bits = sign | 0x7f800000u | (man << 13);
    else if (exp != 0u) bits = sign | ((exp + 112u) << 23) | (man << 13);
    else if (man == 0u) bits = sign;
    else {  /* subnormal: man 2^-24, exact in f32 */
        f = (float)man * 5.9604644775390625e-8f;
        return sign ? -f : f;
    }
    memcpy(&f, &bits, 4);
    return f;
}

static float texel(const void *raw, int fmt, uint64_t i) {
    if (fmt == 0) return (float)((const uint8_t *)raw)[i];
    if (fmt == 3) return (float)((const uint16_t *)raw)[i];
    return half_to_float(((const uint16_t *)raw)[i]);
}

static const int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
static const int ODD[6] = {0, 1, 1, 0, 0, 1};
static const int NTRI[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
/* T[mask][triangle][edge] = 10 a + b */
static const int T[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}},
    {{1, 2, 3}, {0, 0, 0}},       /* 1 */
    {{1, 13, 12}, {0, 0, 0}},     /* 2 */
    {{2, 3, 13}, {2, 13, 12}},    /* 3 */
    {{2, 12, 23}, {0, 0, 0}},     /* 4 */
    {{1, 23, 3}, {1, 12, 23}},    /* 5 */
    {{1, 13, 23}, {1, 23, 2}},    /* 6 */
    {{3, 13, 23}, {0, 0, 0}},     /* 7 */
    {{3, 23, 13}, {0, 0, 0}},     /* 8 */
    {{1, 2, 23}, {1, 23, 13}},    /* 9 */
    {{1, 23, 12}, {1, 3, 23}},    /* 10 */
    {{2, 23, 12}, {0, 0, 0}},     /* 11 */
    {{2, 12, 13}, {2, 13, 3}},    /* 12 */
    {{1, 12, 13}, {0, 0, 0}},     /* 13 */
    {{1, 3, 2}, {0, 0, 0}},       /* 14 */
    {{0, 0, 0}, {0, 0, 0}},
};

/* kinds (may be NULL): [0] cubes skipped for a non-finite corner, [1] all inside, [2] vertices with f == 0, [3] with f == 1,
 * [4 + 16 k + mask] tetrahedra of permutation k with that mask among the cubes that emit.
 * out (may be NULL): the first min(n, cap) triangles, 9 floats each.  Returns n. */
uint64_t mesh_restate(const void *raw, uint32_t nx, uint32_t ny, uint32_t nz, int fmt, const uint32_t *box, float iso_k, float *out, uint64_t cap, uint64_t *kinds) {
    const uint32_t x0 = box[0], y0 = box[1], z0 = box[2], x1 = box[3], y1 = box[4], z1 = box[5];
    const float fn[3] = {(float)nx, (float)ny, (float)nz};
    uint64_t n = 0;
    for (uint32_t z = z0; z + 1u < z1; z++)
        for (uint32_t y = y0; y + 1u < y1; y++)
            for (uint32_t x = x0; x + 1u < x1; x++) {
                float v[2][2][2];  /* [k][j][i] */
                int finite = 1, n_in = 0;
                for (int k = 0; k < 2; k++)
                    for (int j = 0; j < 2; j++)
                        for (int i = 0; i < 2; i++) {
                            const float t = texel(raw, fmt, (uint64_t)(x + i) + (uint64_t)nx * ((uint64_t)(y + j) + (uint64_t)ny * (uint64_t)(z + k)));
                            v[k][j][i] = t;
                            if (isnan(t) || isinf(t)) finite = 0;
                            else if (t >= iso_k) n_in++;
                        }
                if (!finite) { if (kinds) kinds[0]++; continue; }
                if (n_in == 8) { if (kinds) kinds[1]++; continue; }
                if (n_in == 0) continue;
                for (int k = 0; k < 6; k++) {
                    int vert[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {1, 1, 1}};
                    vert[1][PERM[k][0]] = 1;
                    vert[2][PERM[k][0]] = 1;
                    vert[2][PERM[k][1]] = 1;
                    float val[4];
                    int mask = 0;
                    for (int i = 0; i < 4; i++) {
                        val[i] = v[vert[i][2]][vert[i][1]][vert[i][0]];
                        if (val[i] >= iso_k) mask |= 1 << i;
                    }
                    if (kinds) kinds[4 + 16 * k + mask]++;
                    for (int t = 0; t < NTRI[mask]; t++, n++) {
                        float tri[3][3];
                        for (int e = 0; e < 3; e++) {
                            const int a = T[mask][t][e] / 10, b = T[mask][t][e] % 10;
                            const uint32_t A[3] = {x + (uint32_t)vert[a][0], y + (uint32_t)vert[a][1], z + (uint32_t)vert[a][2]};
                            const float f = (iso_k - val[a]) / (val[b] - val[a]);
                            if (kinds && f == 0.0f) kinds[2]++;
                            if (kinds && f == 1.0f) kinds[3]++;
                            const int slot = (ODD[k] && e) ? 3 - e : e;
                            for (int c = 0; c < 3; c++) {
                                const float base = (float)A[c] + 0.5f;
                                const float moved = base + (vert[b][c] > vert[a][c] ? f : 0.0f);
                                tri[slot][c] = moved / fn[c];
                            }
                        }
                        if (out && n < cap) memcpy(out + 9u * n, tri, sizeof(tri));
                    }
                }
            }
    return n;
}
