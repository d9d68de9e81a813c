/* TEST INFRASTRUCTURE: a restatement of NAIVE_TRILINEAR under the runtime transfer function (vk_set_transfer_function), built on
 * the oracle's exported pieces -- vo_ray_naive, vo_intersect_box, vo_sample_trilinear, vo_linear_to_srgb -- and implementing only
 * the loop.  rgba == NULL: the built-in transfer (vo_transfer_alpha + vo_vertigo, composited as the oracle's pixel_naive does), which
 * must reproduce vo_render bit for bit: that keeps this loop honest.  Build with -ffp-contract=off: every fused operation is written. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vokselis_oracle.h"

static void pixel(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
                  uint32_t x, uint32_t y, float dt_scale, const float *T, uint32_t n, float k1, float k2, float *out, uint32_t *steps) {
    float eye[3], dir[3], th[2];
    vo_ray_naive(cam, W, H, x, y, eye, dir);
    vo_intersect_box(eye, dir, 0.0f, 1.0f, th);
    *steps = 0;
    out[0] = out[1] = out[2] = 0.0f;
    out[3] = 1.0f;
    if (th[0] > th[1]) return; /* raycast_naive.wgsl:91-93 */
    th[0] = th[0] > 0.0f ? th[0] : 0.0f;
    const float dtx = 1.0f / ((float)nx * fabsf(dir[0])), dty = 1.0f / ((float)ny * fabsf(dir[1])), dtz = 1.0f / ((float)nz * fabsf(dir[2]));
    const float dt = dt_scale * fminf(dtx, fminf(dty, dtz));
    float p[3] = {eye[0] + th[0] * dir[0], eye[1] + th[0] * dir[1], eye[2] + th[0] * dir[2]};
    const float s[3] = {dir[0] * dt, dir[1] * dt, dir[2] * dt};
    const int raw8 = format == VO_FMT_R8_UNORM;
    const float umax = (float)(n - 1);
    const int imax = (int)n - 2;
    float C[3] = {0.0f, 0.0f, 0.0f}, A = 0.0f;
    uint32_t it = 0;
    for (float t = th[0]; t < th[1]; t = t + dt) {
        int any = 0;
        const float v = vo_sample_trilinear(vol, nx, ny, nz, format, p, VO_FLAG_RAW_UNORM8, &any);
        it++;
        if (!T) {
            const float al = vo_transfer_alpha(v, raw8);
            float rgb[3];
            vo_vertigo(al, rgb);
            const float w = (1.0f - A) * al;
            for (int k = 0; k < 3; k++) C[k] = C[k] + w * rgb[k];
            A = A + w;
        } else {
            float u = fmaf(v, k1, k2);
            u = fminf(fmaxf(u, 0.0f), umax); /* a NaN sample reads entry 0 */
            int i = (int)floorf(u);
            i = i < imax ? i : imax;
            const float f = u - (float)i;
            float c[4];
            for (int k = 0; k < 4; k++) c[k] = fmaf(f, T[4 * (i + 1) + k] - T[4 * i + k], T[4 * i + k]);
            const float w = (1.0f - A) * c[3];
            for (int k = 0; k < 3; k++) C[k] = fmaf(w, c[k], C[k]);
            A = A + w;
        }
        if (A >= 0.95f) break; /* :115-117 */
        p[0] = p[0] + s[0];
        p[1] = p[1] + s[1];
        p[2] = p[2] + s[2];
    }
    for (int k = 0; k < 3; k++) out[k] = vo_linear_to_srgb(C[k]);
    *steps = it;
}

/* The tile [tx, tx + tw) x [ty, ty + th) of a W x H frame into out_rgba [H][W][4] / out_steps [H][W]; k1, k2 as the host computes them
 * (vk_tf.hpp: tf_constants).  Returns 0. */
int tfr_render(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
               uint32_t tx, uint32_t ty, uint32_t tw, uint32_t th, float dt_scale, const float *rgba, uint32_t n, float k1, float k2,
               float *out_rgba, uint32_t *out_steps) {
    for (uint32_t y = ty; y < ty + th && y < H; y++)
        for (uint32_t x = tx; x < tx + tw && x < W; x++) {
            const size_t q = (size_t)y * W + x;
            pixel(cam, vol, nx, ny, nz, format, W, H, x, y, dt_scale, rgba, n, k1, k2, out_rgba + 4 * q, out_steps + q);
        }
    return 0;
}
