/* TEST INFRASTRUCTURE: a restatement of NAIVE_TRILINEAR under a first-hit isosurface with light-direction shadows (vk_set_shadows,
 * DESIGN.md section 17), built on the oracle's exported pieces -- vo_ray_naive, vo_intersect_box, vo_sample_trilinear, vo_f16_to_f32,
 * vo_linear_to_srgb -- and implementing only the primary loop, the bisection, the taps' gradient, the shadow loop and the shade, in f32,
 * in the order the specification writes them.  Every sample's taps are fetched here with the oracle's clamp-to-edge addressing and the
 * lerps redone; on R8 and R16F volumes each sample is held to vo_sample_trilinear bit for bit (a difference fails the render, -2); the
 * oracle has no R16_UNORM format, so there the redone lerps stand alone (the same code, integer taps 0..65535).  Under a clip box
 * intersect_box takes the bounds per axis in the oracle's operations; for the unit cube it is vo_intersect_box itself.  Build with
 * -ffp-contract=off: every fused operation is written; sqrtf is correctly rounded and |N.H|^n is pow() in double, rounded once. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vokselis_oracle.h"

/* flags per pixel, for the conditions the CPU fuzz asserts on the case list */
enum {
    SHR_BOX = 1, SHR_HIT = 2, SHR_FIRST = 4,   /* the primary ray: through the box, hit, hit in its first iteration */
    SHR_CAST = 8,                              /* a shadow ray was cast (lit, not a headlight, shadows set) */
    SHR_SHADOWED = 16,                         /* ... and hit */
    SHR_MISS = 32,                             /* tb0 > tb1 */
    SHR_ZERO = 64,                             /* through the box but ts0 >= tb1: no iteration */
    SHR_NAN_SEEN = 128, SHR_PINF_HIT = 256     /* on the shadow ray: a NaN sample (no hit), a +inf sample (a hit) */
};
enum { FMT_R8 = 0, FMT_R16F = 1, FMT_R16U = 3 };

typedef struct {
    float lx, ly, lz, headlight, ka, kd, ks, n;
} light_t;

typedef struct {
    const void *vol;
    uint32_t nx, ny, nz;
    int format;
} volume_t;

/* Audit hook (tests/fastpath_fuzz.cpp): called with every position whose voxel indices a march looks up, and the indices as the kernels
 * form them before any clamp.  ahead = 1: the position one step past a ray's last sample, which the probe-ahead trip of the kernels has
 * located by then.  NULL (the default): nothing is called. */
void (*shr_lookup_hook)(const float p[3], int ix, int iy, int iz, int ahead) = 0;

static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static int sat_i32(float f) { return (f != f) ? 0 : (f < -2147483648.0f ? INT32_MIN : (f >= 2147483648.0f ? INT32_MAX : (int)f)); }

/* The filtered sample at p with its taps' gradient (g may be NULL).  *bad is set when the value parts from the oracle's. */
static float sample_at(const volume_t *V, const float p[3], float g[3], int *bad) {
    const uint32_t nx = V->nx, ny = V->ny, nz = V->nz;
    const float ux = fmaf(p[0], (float)nx, -0.5f), uy = fmaf(p[1], (float)ny, -0.5f), uz = fmaf(p[2], (float)nz, -0.5f);
    const float flx = floorf(ux), fly = floorf(uy), flz = floorf(uz);
    float fx = ux - flx, fy = uy - fly, fz = uz - flz;
    if (fx >= 1.0f) fx = 0x1.fffffep-1f;
    if (fy >= 1.0f) fy = 0x1.fffffep-1f;
    if (fz >= 1.0f) fz = 0x1.fffffep-1f;
    const int ix = sat_i32(flx), iy = sat_i32(fly), iz = sat_i32(flz);
    if (shr_lookup_hook) shr_lookup_hook(p, ix, iy, iz, 0);
    const int x0 = clampi(ix, 0, (int)nx - 1), x1 = clampi(ix < INT32_MAX ? ix + 1 : ix, 0, (int)nx - 1);
    const int y0 = clampi(iy, 0, (int)ny - 1), y1 = clampi(iy < INT32_MAX ? iy + 1 : iy, 0, (int)ny - 1);
    const int z0 = clampi(iz, 0, (int)nz - 1), z1 = clampi(iz < INT32_MAX ? iz + 1 : iz, 0, (int)nz - 1);
    const size_t sy = nx, sz = (size_t)nx * ny;
    const size_t idx[8] = {x0 + y0 * sy + z0 * sz, x1 + y0 * sy + z0 * sz, x0 + y1 * sy + z0 * sz, x1 + y1 * sy + z0 * sz,
                           x0 + y0 * sy + z1 * sz, x1 + y0 * sy + z1 * sz, x0 + y1 * sy + z1 * sz, x1 + y1 * sy + z1 * sz};
    float t[8];
    for (int k = 0; k < 8; k++)
        t[k] = V->format == FMT_R8 ? (float)((const uint8_t *)V->vol)[idx[k]]
                                   : (V->format == FMT_R16U ? (float)((const uint16_t *)V->vol)[idx[k]] : vo_f16_to_f32(((const uint16_t *)V->vol)[idx[k]]));
    const float dx00 = t[1] - t[0], dx10 = t[3] - t[2], dx01 = t[5] - t[4], dx11 = t[7] - t[6];
    const float c00 = fmaf(fx, dx00, t[0]), c10 = fmaf(fx, dx10, t[2]), c01 = fmaf(fx, dx01, t[4]), c11 = fmaf(fx, dx11, t[6]);
    const float y0d = c10 - c00, y1d = c11 - c01;
    const float l0 = fmaf(fy, y0d, c00), l1 = fmaf(fy, y1d, c01);
    const float r = fmaf(fz, l1 - l0, l0);
    if (V->format != FMT_R16U) {
        int any = 0;
        const float v = vo_sample_trilinear(V->vol, nx, ny, nz, V->format, p, VO_FLAG_RAW_UNORM8, &any);
        if (memcmp(&r, &v, sizeof r) != 0 && !(r != r && v != v)) *bad = 1;
    }
    if (g) {
        const float e0 = fmaf(fy, dx10 - dx00, dx00), e1 = fmaf(fy, dx11 - dx01, dx01);
        g[0] = fmaf(fz, e1 - e0, e0) * (float)nx;
        g[1] = fmaf(fz, y1d - y0d, y0d) * (float)ny;
        g[2] = (l1 - l0) * (float)nz;
    }
    return r;
}

/* intersect_box with bounds per axis (box: lo3 then hi3), in vo_intersect_box's operations; NULL: the unit cube, the oracle's own */
static void intersect(const float o[3], const float d[3], const float *box, float t01[2]) {
    if (!box) {
        vo_intersect_box(o, d, 0.0f, 1.0f, t01);
        return;
    }
    float tmin[3], tmax[3];
    for (int i = 0; i < 3; i++) {
        const float inv = 1.0f / d[i];
        const float a = (box[i] - o[i]) * inv, b = (box[3 + i] - o[i]) * inv;
        tmin[i] = fminf(a, b);
        tmax[i] = fmaxf(a, b);
    }
    t01[0] = fmaxf(tmin[0], fmaxf(tmin[1], tmin[2]));
    t01[1] = fminf(tmax[0], fminf(tmax[1], tmax[2]));
}

static float step_of(const volume_t *V, const float d[3], float dt_scale) {
    const float dtx = 1.0f / ((float)V->nx * fabsf(d[0])), dty = 1.0f / ((float)V->ny * fabsf(d[1])), dtz = 1.0f / ((float)V->nz * fabsf(d[2]));
    return dt_scale * fminf(dtx, fminf(dty, dtz));
}

/* the hook's call for the position a ray stands on when its loop has ended without a hit */
static void looked_ahead(const volume_t *V, const float p[3]) {
    if (!shr_lookup_hook) return;
    const float ux = fmaf(p[0], (float)V->nx, -0.5f), uy = fmaf(p[1], (float)V->ny, -0.5f), uz = fmaf(p[2], (float)V->nz, -0.5f);
    shr_lookup_hook(p, sat_i32(floorf(ux)), sat_i32(floorf(uy)), sat_i32(floorf(uz)), 1);
}

/* The shadow ray of the point q towards Lr (a unit vector): whether it hits; *n: its iterations executed; *flags gains SHR_MISS, SHR_ZERO,
 * SHR_NAN_SEEN, SHR_PINF_HIT. */
static int shadow_walk(const volume_t *V, const float q[3], const float Lr[3], float dt_scale, float bias, float iso_k, const float *box,
                       uint32_t *n_out, uint32_t *flags, int *bad) {
    const float dts = step_of(V, Lr, dt_scale);
    float tb[2];
    intersect(q, Lr, box, tb);
    int shadowed = 0;
    uint32_t n = 0;
    if (tb[0] > tb[1]) {
        *flags |= SHR_MISS;
    } else {
        const float ts0 = fmaxf(fmaxf(tb[0], 0.0f), bias * dts);
        float ps[3] = {fmaf(ts0, Lr[0], q[0]), fmaf(ts0, Lr[1], q[1]), fmaf(ts0, Lr[2], q[2])};
        const float ss[3] = {Lr[0] * dts, Lr[1] * dts, Lr[2] * dts};
        for (float t = ts0; t < tb[1]; t = t + dts) {
            const float v = sample_at(V, ps, NULL, bad);
            n++;
            if (v != v) *flags |= SHR_NAN_SEEN;
            if (v >= iso_k) {
                shadowed = 1;
                if (v == INFINITY) *flags |= SHR_PINF_HIT;
                break;
            }
            ps[0] = ps[0] + ss[0]; ps[1] = ps[1] + ss[1]; ps[2] = ps[2] + ss[2];
        }
        if (n == 0) *flags |= SHR_ZERO;
        if (!shadowed && n != 0) looked_ahead(V, ps); /* (a ray without an iteration looks nothing up) */
    }
    *n_out = n;
    return shadowed;
}

typedef struct {
    float *rgba;
    uint32_t *steps, *flags, *sh_iters;
    float *a, *nl;
} pixel_out;

static int pixel(const vo_camera_uniform *cam, const volume_t *V, uint32_t W, uint32_t H, uint32_t x, uint32_t y, float dt_scale, float iso_k,
                 const float rgb[3], uint32_t refine, const light_t *Lt, const float *shadows, const float *box, pixel_out o) {
    float eye[3], dir[3], th[2];
    int bad = 0;
    vo_ray_naive(cam, W, H, x, y, eye, dir);
    intersect(eye, dir, box, th);
    *o.steps = 0; *o.flags = 0; *o.sh_iters = 0;
    *o.a = 0.0f; *o.nl = 0.0f;
    o.rgba[0] = o.rgba[1] = o.rgba[2] = 0.0f;
    o.rgba[3] = 1.0f;
    if (th[0] > th[1]) return 0;
    *o.flags |= SHR_BOX;
    th[0] = th[0] > 0.0f ? th[0] : 0.0f;
    const float dt = step_of(V, dir, dt_scale);
    float p[3] = {eye[0] + th[0] * dir[0], eye[1] + th[0] * dir[1], eye[2] + th[0] * dir[2]};
    const float s[3] = {dir[0] * dt, dir[1] * dt, dir[2] * dt};
    int hit = 0;
    uint32_t it = 0, j = 0;
    for (float t = th[0]; t < th[1]; t = t + dt) {
        const float v = sample_at(V, p, NULL, &bad);
        it++;
        if (v >= iso_k) { hit = 1; break; }
        p[0] = p[0] + s[0]; p[1] = p[1] + s[1]; p[2] = p[2] + s[2];
        j = j + 1;
    }
    *o.steps = it;
    if (!hit && it != 0) looked_ahead(V, p);
    if (bad) return -2;
    if (!hit) return 0;
    *o.flags |= SHR_HIT;
    float a = 0.0f;
    if (j >= 1) {
        float h = 0.5f;
        for (uint32_t i = 1; i <= refine; i++) {
            const float m = a + h;
            const float q[3] = {fmaf(-m, s[0], p[0]), fmaf(-m, s[1], p[1]), fmaf(-m, s[2], p[2])};
            if (sample_at(V, q, NULL, &bad) >= iso_k) a = m;
            h = h * 0.5f;
        }
    } else {
        *o.flags |= SHR_FIRST;
    }
    *o.a = a;
    float c[3] = {rgb[0], rgb[1], rgb[2]};
    if (Lt) {
        const float q[3] = {fmaf(-a, s[0], p[0]), fmaf(-a, s[1], p[1]), fmaf(-a, s[2], p[2])};
        float g[3];
        (void)sample_at(V, q, g, &bad);
        const float Vw[3] = {-dir[0], -dir[1], -dir[2]};
        const int head = Lt->headlight != 0.0f;
        const float Lr[3] = {head ? Vw[0] : Lt->lx, head ? Vw[1] : Lt->ly, head ? Vw[2] : Lt->lz};
        const float hv[3] = {Lr[0] + Vw[0], Lr[1] + Vw[1], Lr[2] + Vw[2]};
        const float hq = fmaf(hv[2], hv[2], fmaf(hv[1], hv[1], hv[0] * hv[0]));
        float Hr[3] = {Vw[0], Vw[1], Vw[2]};
        if (hq >= FLT_MIN) {
            const float hs = 1.0f / sqrtf(hq);
            for (int k = 0; k < 3; k++) Hr[k] = hv[k] * hs;
        }
        /* the shadow ray */
        float kf = 1.0f;
        if (shadows && !head) {
            *o.flags |= SHR_CAST;
            uint32_t n = 0;
            const int shadowed = shadow_walk(V, q, Lr, dt_scale, shadows[1], iso_k, box, &n, o.flags, &bad);
            *o.sh_iters = n;
            if (shadowed) {
                *o.flags |= SHR_SHADOWED;
                kf = 1.0f - shadows[0];
            }
        }
        /* the shade: diff, spec as lit_shade computes them, k on the diffuse and specular terms */
        const float gq = fmaf(g[2], g[2], fmaf(g[1], g[1], g[0] * g[0]));
        float diff = 1.0f, spec = 0.0f;
        if (gq >= FLT_MIN && gq <= FLT_MAX) {
            const float gs = 1.0f / sqrtf(gq);
            const float N[3] = {g[0] * gs, g[1] * gs, g[2] * gs};
            const float nl = fmaf(N[2], Lr[2], fmaf(N[1], Lr[1], N[0] * Lr[0]));
            *o.nl = -nl; /* the outward normal is -g / |g| (values rise into the material): > 0 faces the light */
            diff = fabsf(nl);
            const float nh = fabsf(fmaf(N[2], Hr[2], fmaf(N[1], Hr[1], N[0] * Hr[0])));
            spec = (float)pow((double)nh, (double)Lt->n);
        } else {
            *o.nl = NAN; /* no gradient */
        }
        const float kd_diff = Lt->kd * diff, ks_spec = Lt->ks * spec;
        const float kd_k = kd_diff * kf;
        const float f = Lt->ka + kd_k, sp = ks_spec * kf;
        for (int k = 0; k < 3; k++) {
            const float cf = c[k] * f;
            c[k] = cf + sp;
        }
    }
    if (bad) return -2;
    for (int k = 0; k < 3; k++) o.rgba[k] = vo_linear_to_srgb(c[k]);
    return 0;
}

/* One shadow ray on its own (the audit's secondary rays): from q towards the unit vector L, bias in steps, the unit cube.  Returns whether it
 * hit, -2 as shr_render; *n_out: its iterations executed. */
int shr_shadow_ray(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, const float q[3], const float L[3], float dt_scale,
                   float bias, float iso_k, uint32_t *n_out) {
    const volume_t V = {vol, nx, ny, nz, format};
    uint32_t flags = 0;
    int bad = 0;
    const int shadowed = shadow_walk(&V, q, L, dt_scale, bias, iso_k, NULL, n_out, &flags, &bad);
    return bad ? -2 : shadowed;
}

/* The tile [tx, tx + tw) x [ty, ty + th) of a W x H frame.  format: 0 R8, 1 R16F, 3 R16_UNORM; iso_k on the kernel's scale; light: 8 floats
 * (light_t) or NULL; shadows: (strength, bias) or NULL; box: lo3, hi3 or NULL.  Outputs [H][W] (rgba: [H][W][4]): steps (the primary
 * ray's iterations), a (the refined distance back), flags (above), sh_iters (the shadow ray's iterations executed), nl (the outward
 * normal's N.L; NaN without a gradient; 0 where nothing was shaded).  Returns 0, or -2 (see sample_at). */
int shr_render(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
               uint32_t tx, uint32_t ty, uint32_t tw, uint32_t th, float dt_scale, float iso_k, const float *rgb, uint32_t refine,
               const float *light, const float *shadows, const float *box, float *out_rgba, uint32_t *out_steps, float *out_a, uint32_t *out_flags,
               uint32_t *out_sh_iters, float *out_nl) {
    light_t Lt;
    if (light) memcpy(&Lt, light, sizeof Lt);
    const volume_t V = {vol, nx, ny, nz, format};
    for (uint32_t y = ty; y < ty + th && y < H; y++)
        for (uint32_t x = tx; x < tx + tw && x < W; x++) {
            const size_t q = (size_t)y * W + x;
            const pixel_out o = {out_rgba + 4 * q, out_steps + q, out_flags + q, out_sh_iters + q, out_a + q, out_nl + q};
            const int rc = pixel(cam, &V, W, H, x, y, dt_scale, iso_k, rgb, refine, light ? &Lt : NULL, shadows, box, o);
            if (rc) return rc;
        }
    return 0;
}
