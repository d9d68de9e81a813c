/* TEST INFRASTRUCTURE: a restatement of NAIVE_TRILINEAR under first-hit isosurface rendering (vk_set_isosurface),
 * built on the oracle's exported pieces -- vo_ray_naive, vo_intersect_box, vo_sample_trilinear, vo_f16_to_f32, vo_linear_to_srgb -- and
 * implementing only the loop, the bisection, the taps' gradient and the shade, in f32, in the order the specification writes them.  The
 * sample value is the oracle's; for the shaded sample the taps are fetched here with the oracle's clamp-to-edge addressing and the lerps
 * redone, and a sample whose lerps disagree with vo_sample_trilinear fails the render (-2).  Build with -ffp-contract=off: every fused
 * operation is written; sqrtf is correctly rounded and |N.H|^n is pow() in double, rounded once. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vokselis_oracle.h"

/* flags per pixel, for the conditions the CPU fuzz asserts on the case list */
enum { ISOR_BOX = 1, ISOR_HIT = 2, ISOR_FIRST = 4, ISOR_NAN_SEEN = 8, ISOR_PINF_HIT = 16, ISOR_EQUAL = 32 };

/* light[8]: lx, ly, lz (unit, world), headlight (0 / 1), ka, kd, ks, shininess */
typedef struct {
    float lx, ly, lz, headlight, ka, kd, ks, n;
} light_t;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int sat_i32(float f) { return (f != f) ? 0 : (f < -2147483648.0f ? INT32_MIN : (f >= 2147483648.0f ? INT32_MAX : (int)f)); }

static float value_at(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, const float p[3]) {
    int any = 0;
    return vo_sample_trilinear(vol, nx, ny, nz, format, p, VO_FLAG_RAW_UNORM8, &any);
}

/* The world gradient g of the sample at p.  Returns 0, or -2 when the redone lerps part from the oracle's value. */
static int gradient_at(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, const float p[3], float g[3]) {
    const float v = value_at(vol, nx, ny, nz, format, p);
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
                 uint32_t x, uint32_t y, float dt_scale, float iso_k, const float rgb[3], uint32_t refine, const light_t *Lt, float *out,
                 uint32_t *steps, float *a_out, uint32_t *flags) {
    float eye[3], dir[3], th[2];
    vo_ray_naive(cam, W, H, x, y, eye, dir);
    vo_intersect_box(eye, dir, 0.0f, 1.0f, th);
    *steps = 0;
    *a_out = 0.0f;
    *flags = 0;
    out[0] = out[1] = out[2] = 0.0f;
    out[3] = 1.0f;
    if (th[0] > th[1]) return 0; /* raycast_naive.wgsl:91-93 */
    *flags |= ISOR_BOX;
    th[0] = th[0] > 0.0f ? th[0] : 0.0f;
    const float dtx = 1.0f / ((float)nx * fabsf(dir[0])), dty = 1.0f / ((float)ny * fabsf(dir[1])), dtz = 1.0f / ((float)nz * fabsf(dir[2]));
    const float dt = dt_scale * fminf(dtx, fminf(dty, dtz));
    float p[3] = {eye[0] + th[0] * dir[0], eye[1] + th[0] * dir[1], eye[2] + th[0] * dir[2]};
    const float s[3] = {dir[0] * dt, dir[1] * dt, dir[2] * dt};
    int hit = 0;
    uint32_t it = 0, j = 0;
    for (float t = th[0]; t < th[1]; t = t + dt) {
        const float v = value_at(vol, nx, ny, nz, format, p);
        it++;
        if (v != v) *flags |= ISOR_NAN_SEEN;
        if (v >= iso_k) {
            hit = 1;
            if (v == INFINITY) *flags |= ISOR_PINF_HIT;
            if (v == iso_k) *flags |= ISOR_EQUAL;
            break;
        }
        p[0] = p[0] + s[0];
        p[1] = p[1] + s[1];
        p[2] = p[2] + s[2];
        j = j + 1;
    }
    *steps = it;
    if (!hit) return 0;
    *flags |= ISOR_HIT;
    float a = 0.0f;
    if (j >= 1) {
        float h = 0.5f;
        for (uint32_t i = 1; i <= refine; i++) {
            const float m = a + h;
            const float q[3] = {fmaf(-m, s[0], p[0]), fmaf(-m, s[1], p[1]), fmaf(-m, s[2], p[2])};
            if (value_at(vol, nx, ny, nz, format, q) >= iso_k) a = m;
            h = h * 0.5f;
        }
    } else {
        *flags |= ISOR_FIRST;
    }
    *a_out = a;
    float c[3] = {rgb[0], rgb[1], rgb[2]};
    if (Lt) {
        const float q[3] = {fmaf(-a, s[0], p[0]), fmaf(-a, s[1], p[1]), fmaf(-a, s[2], p[2])};
        float g[3];
        if (gradient_at(vol, nx, ny, nz, format, q, g)) return -2;
        /* the ray's light and half vectors */
        const float V[3] = {-dir[0], -dir[1], -dir[2]};
        const int head = Lt->headlight != 0.0f;
        const float Lr[3] = {head ? V[0] : Lt->lx, head ? V[1] : Lt->ly, head ? V[2] : Lt->lz};
        const float hv[3] = {Lr[0] + V[0], Lr[1] + V[1], Lr[2] + V[2]};
        const float hq = fmaf(hv[2], hv[2], fmaf(hv[1], hv[1], hv[0] * hv[0]));
        float Hr[3] = {V[0], V[1], V[2]};
        if (hq >= FLT_MIN) {
            const float hs = 1.0f / sqrtf(hq);
            for (int k = 0; k < 3; k++) Hr[k] = hv[k] * hs;
        }
        shade(Lt, Lr, Hr, g, c);
    }
    for (int k = 0; k < 3; k++) out[k] = vo_linear_to_srgb(c[k]);
    return 0;
}

/* The tile [tx, tx + tw) x [ty, ty + th) of a W x H frame into out_rgba [H][W][4], out_steps, out_a (the refined a) and out_flags
 * [H][W]; iso_k on the kernel's scale; light: 8 floats (see light_t) or NULL.  Returns 0, or -2 (see gradient_at). */
int isor_render(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
                uint32_t tx, uint32_t ty, uint32_t tw, uint32_t th, float dt_scale, float iso_k, const float *rgb, uint32_t refine,
                const float *light, float *out_rgba, uint32_t *out_steps, float *out_a, uint32_t *out_flags) {
    light_t Lt;
    if (light) memcpy(&Lt, light, sizeof Lt);
    for (uint32_t y = ty; y < ty + th && y < H; y++)
        for (uint32_t x = tx; x < tx + tw && x < W; x++) {
            const size_t q = (size_t)y * W + x;
            const int rc = pixel(cam, vol, nx, ny, nz, format, W, H, x, y, dt_scale, iso_k, rgb, refine, light ? &Lt : NULL, out_rgba + 4 * q,
                                 out_steps + q, out_a + q, out_flags + q);
            if (rc) return rc;
        }
    return 0;
}
