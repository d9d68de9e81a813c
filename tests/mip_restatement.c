/* TEST INFRASTRUCTURE: a restatement of NAIVE_TRILINEAR under the maximum-intensity projection (vk_set_projection(VK_PROJ_MAX),
 * DESIGN.md section 12), built on the oracle's exported pieces -- vo_ray_naive, vo_intersect_box, vo_sample_trilinear,
 * vo_linear_to_srgb -- and implementing only the loop and the lookup, in f32, in the order the specification writes them.
 * Build with -ffp-contract=off: every fused operation is written. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vokselis_oracle.h"

/* flags per pixel, for the conditions the CPU fuzz asserts on the case list */
enum { MIPR_HIT = 1, MIPR_BROKE = 2, MIPR_MAX_AT_LAST = 4, MIPR_NAN_SEEN = 8, MIPR_PINF_SEEN = 16 };

static void pixel(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
                  uint32_t x, uint32_t y, float dt_scale, const float *T, uint32_t n, float k1, float k2, float *out, uint32_t *steps,
                  float *u_out, uint32_t *flags) {
    float eye[3], dir[3], th[2];
    vo_ray_naive(cam, W, H, x, y, eye, dir);
    vo_intersect_box(eye, dir, 0.0f, 1.0f, th);
    *steps = 0;
    *u_out = 0.0f;
    *flags = 0;
    out[0] = out[1] = out[2] = 0.0f;
    out[3] = 1.0f;
    if (th[0] > th[1]) return;
    *flags |= MIPR_HIT;
    th[0] = th[0] > 0.0f ? th[0] : 0.0f;
    const float dtx = 1.0f / ((float)nx * fabsf(dir[0])), dty = 1.0f / ((float)ny * fabsf(dir[1])), dtz = 1.0f / ((float)nz * fabsf(dir[2]));
    const float dt = dt_scale * fminf(dtx, fminf(dty, dtz));
    float p[3] = {eye[0] + th[0] * dir[0], eye[1] + th[0] * dir[1], eye[2] + th[0] * dir[2]};
    const float s[3] = {dir[0] * dt, dir[1] * dt, dir[2] * dt};
    const float umax = (float)(n - 1);
    const int imax = (int)n - 2;
    float U = 0.0f;
    uint32_t it = 0, last_rise = 0;
    for (float t = th[0]; t < th[1]; t = t + dt) {
        int any = 0;
        const float v = vo_sample_trilinear(vol, nx, ny, nz, format, p, VO_FLAG_RAW_UNORM8, &any);
        it++;
        if (v != v) *flags |= MIPR_NAN_SEEN;
        if (v == INFINITY) *flags |= MIPR_PINF_SEEN;
        float u = fmaf(v, k1, k2);
        u = fminf(fmaxf(u, 0.0f), umax); /* tf_u: a NaN sample gives 0 */
        const float U1 = fmaxf(U, u) + 0.0f; /* +0 whenever it compares equal to zero */
        if (U1 > U) last_rise = it;
        U = U1;
        if (U >= umax) {
            *flags |= MIPR_BROKE;
            break;
        }
        p[0] = p[0] + s[0];
        p[1] = p[1] + s[1];
        p[2] = p[2] + s[2];
    }
    if (it > 1 && last_rise == it && !(*flags & MIPR_BROKE)) *flags |= MIPR_MAX_AT_LAST; /* the loop ran out with its maximum in the last iteration */
    int i = (int)floorf(U);
    i = i < imax ? i : imax;
    const float f = U - (float)i;
    for (int k = 0; k < 3; k++) out[k] = vo_linear_to_srgb(fmaf(f, T[4 * (i + 1) + k] - T[4 * i + k], T[4 * i + k]));
    *steps = it;
    *u_out = U;
}

/* The tile [tx, tx + tw) x [ty, ty + th) of a W x H frame into out_rgba [H][W][4], out_steps, out_u (the ray's U) and out_flags [H][W];
 * rgba: the n entries of the table (the caller passes the grey ramp when none is set); k1, k2 as the host computes them.  Returns 0. */
int mipr_render(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
                uint32_t tx, uint32_t ty, uint32_t tw, uint32_t th, float dt_scale, const float *rgba, uint32_t n, float k1, float k2,
                float *out_rgba, uint32_t *out_steps, float *out_u, uint32_t *out_flags) {
    for (uint32_t y = ty; y < ty + th && y < H; y++)
        for (uint32_t x = tx; x < tx + tw && x < W; x++) {
            const size_t q = (size_t)y * W + x;
            pixel(cam, vol, nx, ny, nz, format, W, H, x, y, dt_scale, rgba, n, k1, k2, out_rgba + 4 * q, out_steps + q, out_u + q, out_flags + q);
        }
    return 0;
}
