/* TEST INFRASTRUCTURE: a restatement of the slice pass (vk_render_slice), built on the oracle's exported pieces --
 * vo_sample_trilinear, vo_f16_to_f32, vo_linear_to_srgb -- and implementing only the plane, the inside test, the slab and the lookup, in
 * f32, in the order the specification writes them.  Every sample's taps are fetched here with the oracle's clamp-to-edge addressing and
 * the lerps redone; on R8 and R16F volumes each sample is held to vo_sample_trilinear bit for bit (a difference fails the render, -2);
 * the oracle has no R16_UNORM format, so there the redone lerps stand alone (the same code, integer taps 0..65535).
 * Build with -ffp-contract=off: every fused operation is written. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vokselis_oracle.h"

/* flags per pixel, for the conditions the CPU fuzz asserts on the case list */
enum { SR_INSIDE = 1, SR_FACE = 2, SR_CLAMPED = 4, SR_NAN_PASSED = 8, SR_ALL_NAN = 16, SR_MEAN_ROUNDED = 32 };
enum { FMT_R8 = 0, FMT_R16F = 1, FMT_R16U = 3 };
enum { SLAB_MAX = 0, SLAB_MIN = 1, SLAB_MEAN = 2 };

typedef struct {
    const void *vol;
    uint32_t nx, ny, nz;
    int format;
} volume_t;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int sat_i32(float f) { return (f != f) ? 0 : (f < -2147483648.0f ? INT32_MIN : (f >= 2147483648.0f ? INT32_MAX : (int)f)); }

/* The filtered sample at p.  *bad is set when the value parts from the oracle's; *clamped when a texel index was clamped to the edge. */
static float sample_at(const volume_t *V, const float p[3], int *bad, int *clamped) {
    const uint32_t nx = V->nx, ny = V->ny, nz = V->nz;
    const float ux = fmaf(p[0], (float)nx, -0.5f), uy = fmaf(p[1], (float)ny, -0.5f), uz = fmaf(p[2], (float)nz, -0.5f);
    const float flx = floorf(ux), fly = floorf(uy), flz = floorf(uz);
    float fx = ux - flx, fy = uy - fly, fz = uz - flz;
    if (fx >= 1.0f) fx = 0x1.fffffep-1f;
    if (fy >= 1.0f) fy = 0x1.fffffep-1f;
    if (fz >= 1.0f) fz = 0x1.fffffep-1f;
    if (isinf(ux)) fx = 0.0f; /* v_fract_f32 of an infinity (never reached: |P| stays far below the f32 range) */
    if (isinf(uy)) fy = 0.0f;
    if (isinf(uz)) fz = 0.0f;
    const int ix = sat_i32(flx), iy = sat_i32(fly), iz = sat_i32(flz);
    const int ix1 = ix < INT32_MAX ? ix + 1 : ix, iy1 = iy < INT32_MAX ? iy + 1 : iy, iz1 = iz < INT32_MAX ? iz + 1 : iz;
    const int x0 = clampi(ix, 0, (int)nx - 1), x1 = clampi(ix1, 0, (int)nx - 1);
    const int y0 = clampi(iy, 0, (int)ny - 1), y1 = clampi(iy1, 0, (int)ny - 1);
    const int z0 = clampi(iz, 0, (int)nz - 1), z1 = clampi(iz1, 0, (int)nz - 1);
    if (x0 != ix || x1 != ix1 || y0 != iy || y1 != iy1 || z0 != iz || z1 != iz1) *clamped = 1;
    const size_t sy = nx, sz = (size_t)nx * ny;
    const size_t idx[8] = {x0 + y0 * sy + z0 * sz, x1 + y0 * sy + z0 * sz, x0 + y1 * sy + z0 * sz, x1 + y1 * sy + z0 * sz,
                           x0 + y0 * sy + z1 * sz, x1 + y0 * sy + z1 * sz, x0 + y1 * sy + z1 * sz, x1 + y1 * sy + z1 * sz};
    float t[8];
    for (int k = 0; k < 8; k++)
        t[k] = V->format == FMT_R8 ? (float)((const uint8_t *)V->vol)[idx[k]]
                                   : (V->format == FMT_R16U ? (float)((const uint16_t *)V->vol)[idx[k]] : vo_f16_to_f32(((const uint16_t *)V->vol)[idx[k]]));
    const float c00 = fmaf(fx, t[1] - t[0], t[0]), c10 = fmaf(fx, t[3] - t[2], t[2]), c01 = fmaf(fx, t[5] - t[4], t[4]), c11 = fmaf(fx, t[7] - t[6], t[6]);
    const float l0 = fmaf(fy, c10 - c00, c00), l1 = fmaf(fy, c11 - c01, c01);
    const float r = fmaf(fz, l1 - l0, l0);
    if (V->format != FMT_R16U) {
        int any = 0;
        const float v = vo_sample_trilinear(V->vol, nx, ny, nz, V->format, p, VO_FLAG_RAW_UNORM8, &any);
        if (memcmp(&r, &v, sizeof r) != 0 && !(r != r && v != v)) *bad = 1;
    }
    return r;
}

/* plane: origin3, du3, dv3, dn3; box: lo3, hi3; T: n RGBA entries.  rgba: the pixel's 4 floats; val: (x, weight); pos: P. */
static int pixel(const volume_t *V, const float *plane, uint32_t samples, int reduce, float rn, const float *box, const float *T, uint32_t n,
                 float k1, float k2, uint32_t px, uint32_t py, float *rgba, float *val, float *pos, uint32_t *flags) {
    const float *origin = plane, *du = plane + 3, *dv = plane + 6, *dn = plane + 9;
    float P[3];
    int bad = 0, clamped = 0;
    *flags = 0;
    for (int c = 0; c < 3; c++) pos[c] = P[c] = fmaf((float)py, dv[c], fmaf((float)px, du[c], origin[c]));
    int inside = 1, face = 0;
    for (int c = 0; c < 3; c++) {
        if (!(box[c] <= P[c] && P[c] <= box[3 + c])) inside = 0;
        if (P[c] == box[c] || P[c] == box[3 + c]) face = 1;
    }
    rgba[0] = rgba[1] = rgba[2] = 0.0f;
    rgba[3] = 1.0f;
    val[0] = 0.0f;
    val[1] = 0.0f;
    if (!inside) return 0;
    *flags |= SR_INSIDE | (face ? SR_FACE : 0);
    float x;
    if (samples == 1) {
        x = sample_at(V, P, &bad, &clamped);
    } else {
        float M = reduce == SLAB_MAX ? -INFINITY : (reduce == SLAB_MIN ? INFINITY : 0.0f);
        uint32_t nans = 0;
        for (uint32_t k = 0; k < samples; k++) {
            const float w = (float)k - 0.5f * (float)(samples - 1);
            const float Pk[3] = {fmaf(w, dn[0], P[0]), fmaf(w, dn[1], P[1]), fmaf(w, dn[2], P[2])};
            int cl = 0;
            const float xk = sample_at(V, Pk, &bad, &cl);
            if (cl) *flags |= SR_CLAMPED;
            if (xk != xk) nans++;
            if (reduce == SLAB_MAX) M = (xk > M) ? xk : M;
            else if (reduce == SLAB_MIN) M = (xk < M) ? xk : M;
            else {
                const float s = M + xk;
                if ((double)M + (double)xk != (double)s) *flags |= SR_MEAN_ROUNDED;
                M = s;
            }
        }
        if (reduce != SLAB_MEAN && nans == samples) *flags |= SR_ALL_NAN;
        if (reduce != SLAB_MEAN && nans > 0 && nans < samples) *flags |= SR_NAN_PASSED;
        x = reduce == SLAB_MEAN ? M * rn : M;
    }
    if (bad) return -2;
    /* mip_update(+0, x): u replaces +0 only when u > 0 */
    const float umax = (float)(n - 1);
    const int imax = (int)n - 2;
    const float u = fmaf(x, k1, k2);
    const float U = fminf(u > 0.0f ? u : 0.0f, umax);
    int i = (int)floorf(U);
    i = i < imax ? i : imax;
    const float f = U - (float)i;
    for (int k = 0; k < 3; k++) rgba[k] = vo_linear_to_srgb(fmaf(f, T[4 * (i + 1) + k] - T[4 * i + k], T[4 * i + k]));
    val[0] = x;
    val[1] = 1.0f;
    return 0;
}

/* The tile [tx, tx + tw) x [ty, ty + th) of a W x H frame (the origin may be negative: the part inside the frame is rendered).  format: 0
 * R8, 1 R16F, 3 R16_UNORM; k1, k2, rn as the host forms them; rgba: the n entries of the table (the caller passes the grey ramp when none
 * is set).  Outputs [H][W]: out_rgba (4 f32), out_val (2 f32), out_pos (3 f32), out_flags.  Pixels outside the tile are left as they are.
 * Returns 0, or -2 (see sample_at). */
int slicer_render(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H, int32_t tx, int32_t ty, uint32_t tw,
                  uint32_t th, const float *plane, uint32_t samples, int reduce, float rn, const float *box, const float *rgba, uint32_t n, float k1,
                  float k2, float *out_rgba, float *out_val, float *out_pos, uint32_t *out_flags) {
    const volume_t V = {vol, nx, ny, nz, format};
    const int64_t x1 = (int64_t)tx + tw, y1 = (int64_t)ty + th;
    for (int64_t y = ty < 0 ? 0 : ty; y < y1 && y < (int64_t)H; y++)
        for (int64_t x = tx < 0 ? 0 : tx; x < x1 && x < (int64_t)W; x++) {
            const size_t q = (size_t)y * W + (size_t)x;
            const int rc = pixel(&V, plane, samples, reduce, rn, box, rgba, n, k1, k2, (uint32_t)x, (uint32_t)y, out_rgba + 4 * q, out_val + 2 * q,
                                 out_pos + 3 * q, out_flags + q);
            if (rc) return rc;
        }
    return 0;
}
