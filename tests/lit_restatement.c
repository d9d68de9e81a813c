/* TEST INFRASTRUCTURE: a restatement of NAIVE_TRILINEAR under a runtime transfer function with gradient lighting (vk_set_lighting), built
 * on the oracle's exported pieces -- vo_ray_naive, vo_intersect_box, vo_sample_trilinear, vo_f16_to_f32, vo_linear_to_srgb -- and
 * implementing only the loop, the taps' gradient and the shade.  The sample value is the oracle's; the taps are
 * fetched here with the oracle's clamp-to-edge addressing and the lerps redone, and a sample whose lerps disagree with vo_sample_trilinear
 * fails the render (-2).  Build with -ffp-contract=off: every fused operation is written; sqrtf is correctly rounded and |N.H|^n is
 * pow() in double, rounded once. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vokselis_oracle.h"

/* light[8]: lx, ly, lz (unit, world), headlight (0 / 1), ka, kd, ks, shininess */
typedef struct {
    float lx, ly, lz, headlight, ka, kd, ks, n;
} light_t;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static int sat_i32(float f) { return (f != f) ? 0 : (f < -2147483648.0f ? INT32_MIN : (f >= 2147483648.0f ? INT32_MAX : (int)f)); }

/* The sample at p: value (the oracle's) and world gradient g.  Returns 0, or -2 when the redone lerps part from the oracle's value. */
static int sample_lit(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, const float p[3], float *value, float g[3]) {
    int any = 0;
    const float v = vo_sample_trilinear(vol, nx, ny, nz, format, p, VO_FLAG_RAW_UNORM8, &any);
    const float ux = fmaf(p[0], (float)nx, -0.5f), uy = fmaf(p[1], (float)ny, -0.5f), uz = fmaf(p[2], (float)nz, -0.5f);
    const float flx = floorf(ux), fly = floorf(uy), flz = floorf(uz);
    float fx = ux - flx, fy = uy - fly, fz = uz - flz;
    if (fx >= 1.0f) fx = 0x1.fffffep-1f;
    if (fy >= 1.0f) fy = 0x1.fffffep-1f;
    if (fz >= 1.0f) fz = 0x1.fffffep-1f;
    const int ix = sat_i32(flx), iy = sat_i32(fly), iz = sat_i32(flz);
    const int x0 = clampi(ix, 0, (int)nx - 1), x1 = clampi(ix < INT32_MAX ? ix + 1 : ix, 0, (int)nx - 1);
    const int y0 = clampi(iy, 0, (int)ny - 1), y1 = clampi(iy < INT32_MAX ? iy + 1 : iy, 0, (int)ny - 1);
    const int z0 = clampi(iz, 0, (int)nz - 1), z1 = clampi(iz < INT32_MAX ? iz + 1 : iz, 0, (int)nz - 1);
    const size_t sy = nx, sz = (size_t)nx * ny;
    const size_t idx[8] = {x0 + y0 * sy + z0 * sz, x1 + y0 * sy + z0 * sz, x0 + y1 * sy + z0 * sz, x1 + y1 * sy + z0 * sz,
                           x0 + y0 * sy + z1 * sz, x1 + y0 * sy + z1 * sz, x0 + y1 * sy + z1 * sz, x1 + y1 * sy + z1 * sz};
    float t[8];
    for (int k = 0; k < 8; k++)
        t[k] = format == VO_FMT_R8_UNORM ? (float)((const uint8_t *)vol)[idx[k]] : vo_f16_to_f32(((const uint16_t *)vol)[idx[k]]);
    const float dx00 = t[1] - t[0], dx10 = t[3] - t[2], dx01 = t[5] - t[4], dx11 = t[7] - t[6];
    const float c00 = fmaf(fx, dx00, t[0]), c10 = fmaf(fx, dx10, t[2]), c01 = fmaf(fx, dx01, t[4]), c11 = fmaf(fx, dx11, t[6]);
    const float y0d = c10 - c00, y1d = c11 - c01;
    const float l0 = fmaf(fy, y0d, c00), l1 = fmaf(fy, y1d, c01);
    const float r = fmaf(fz, l1 - l0, l0);
    if (memcmp(&r, &v, sizeof r) != 0 && !(r != r && v != v)) return -2;
    const float e0 = fmaf(fy, dx10 - dx00, dx00), e1 = fmaf(fy, dx11 - dx01, dx01);
    g[0] = fmaf(fz, e1 - e0, e0) * (float)nx;
    g[1] = fmaf(fz, y1d - y0d, y0d) * (float)ny;
    g[2] = (l1 - l0) * (float)nz;
    *value = v;
    return 0;
}

static void shade(const light_t *Lt, const float Lr[3], const float Hr[3], const float g[3], float c[3]) {
    const float q = fmaf(g[2], g[2], fmaf(g[1], g[1], g[0] * g[0]));
    float diff = 1.0f, spec = 0.0f;
    if (q >= FLT_MIN && q <= FLT_MAX) {
        const float s = 1.0f / sqrtf(q);
        const float N[3] = {g[0] * s, g[1] * s, g[2] * s};
        diff = fabsf(fmaf(N[2], Lr[2], fmaf(N[1], Lr[1], N[0] * Lr[0])));
        const float nh = fabsf(fmaf(N[2], Hr[2], fmaf(N[1], Hr[1], N[0] * Hr[0])));
        spec = (float)pow((double)nh, (double)Lt->n);
    }
    const float kd_diff = Lt->kd * diff;
    const float f = Lt->ka + kd_diff, sp = Lt->ks * spec;
    for (int k = 0; k < 3; k++) {
        const float cf = c[k] * f;
        c[k] = cf + sp;
    }
}

static int pixel(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
                 uint32_t x, uint32_t y, float dt_scale, const float *T, uint32_t n, float k1, float k2, const light_t *Lt, float *out,
                 uint32_t *steps) {
    float eye[3], dir[3], th[2];
    vo_ray_naive(cam, W, H, x, y, eye, dir);
    vo_intersect_box(eye, dir, 0.0f, 1.0f, th);
    *steps = 0;
    out[0] = out[1] = out[2] = 0.0f;
    out[3] = 1.0f;
    if (th[0] > th[1]) return 0; /* raycast_naive.wgsl:91-93 */
    th[0] = th[0] > 0.0f ? th[0] : 0.0f;
    /* the ray's light and half vectors */
    const float V[3] = {-dir[0], -dir[1], -dir[2]};
    const int head = Lt && Lt->headlight != 0.0f;
    const float Lr[3] = {head ? V[0] : (Lt ? Lt->lx : 0.0f), head ? V[1] : (Lt ? Lt->ly : 0.0f), head ? V[2] : (Lt ? Lt->lz : 0.0f)};
    const float h[3] = {Lr[0] + V[0], Lr[1] + V[1], Lr[2] + V[2]};
    const float hq = fmaf(h[2], h[2], fmaf(h[1], h[1], h[0] * h[0]));
    float Hr[3] = {V[0], V[1], V[2]};
    if (hq >= FLT_MIN) {
        const float s = 1.0f / sqrtf(hq);
        for (int k = 0; k < 3; k++) Hr[k] = h[k] * s;
    }
    const float dtx = 1.0f / ((float)nx * fabsf(dir[0])), dty = 1.0f / ((float)ny * fabsf(dir[1])), dtz = 1.0f / ((float)nz * fabsf(dir[2]));
    const float dt = dt_scale * fminf(dtx, fminf(dty, dtz));
    float p[3] = {eye[0] + th[0] * dir[0], eye[1] + th[0] * dir[1], eye[2] + th[0] * dir[2]};
    const float s[3] = {dir[0] * dt, dir[1] * dt, dir[2] * dt};
    const float umax = (float)(n - 1);
    const int imax = (int)n - 2;
    float C[3] = {0.0f, 0.0f, 0.0f}, A = 0.0f;
    uint32_t it = 0;
    for (float t = th[0]; t < th[1]; t = t + dt) {
        float v, g[3];
        if (sample_lit(vol, nx, ny, nz, format, p, &v, g)) return -2;
        it++;
        float u = fmaf(v, k1, k2);
        u = fminf(fmaxf(u, 0.0f), umax); /* a NaN sample reads entry 0 */
        int i = (int)floorf(u);
        i = i < imax ? i : imax;
        const float f = u - (float)i;
        float c[4];
        for (int k = 0; k < 4; k++) c[k] = fmaf(f, T[4 * (i + 1) + k] - T[4 * i + k], T[4 * i + k]);
        if (Lt) shade(Lt, Lr, Hr, g, c);
        const float w = (1.0f - A) * c[3];
        for (int k = 0; k < 3; k++) C[k] = fmaf(w, c[k], C[k]);
        A = A + w;
        if (A >= 0.95f) break; /* :115-117 */
        p[0] = p[0] + s[0];
        p[1] = p[1] + s[1];
        p[2] = p[2] + s[2];
    }
    for (int k = 0; k < 3; k++) out[k] = vo_linear_to_srgb(C[k]);
    *steps = it;
    return 0;
}

/* The tile [tx, tx + tw) x [ty, ty + th) of a W x H frame into out_rgba [H][W][4] / out_steps [H][W]; k1, k2 as the host computes them
 * (vk_tf.hpp: tf_constants); light: 8 floats (see light_t) or NULL for the unlit table.  Returns 0, or -2 (see sample_lit). */
int litr_render(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
                uint32_t tx, uint32_t ty, uint32_t tw, uint32_t th, float dt_scale, const float *rgba, uint32_t n, float k1, float k2,
                const float *light, float *out_rgba, uint32_t *out_steps) {
    light_t Lt;
    if (light) memcpy(&Lt, light, sizeof Lt);
    for (uint32_t y = ty; y < ty + th && y < H; y++)
        for (uint32_t x = tx; x < tx + tw && x < W; x++) {
            const size_t q = (size_t)y * W + x;
            const int rc = pixel(cam, vol, nx, ny, nz, format, W, H, x, y, dt_scale, rgba, n, k1, k2, light ? &Lt : NULL, out_rgba + 4 * q, out_steps + q);
            if (rc) return rc;
        }
    return 0;
}

/* The value (vo_sample_trilinear, raw u8 scale) and the world gradient of the sample at p.  Returns 0, or -2 (see sample_lit). */
int litr_sample(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, const float *p, float *value, float *g) {
    return sample_lit(vol, nx, ny, nz, format, p, value, g);
}
