/* TEST INFRASTRUCTURE: a restatement of the geometry pass of the first-hit isosurface (vk_render_geometry), built
 * on the oracle's exported pieces -- vo_ray_naive, vo_intersect_box, vo_sample_trilinear, vo_f16_to_f32 -- and implementing only the
 * primary loop, the bisection (always run), the taps' gradient and the distance along the ray, in f32, in the order the specification
 * writes them.  Every sample's taps are fetched here with the oracle's clamp-to-edge addressing and the lerps redone; on R8 and R16F
 * volumes each sample is held to vo_sample_trilinear bit for bit (a difference fails the render, -2); the oracle has no R16_UNORM format,
 * so there the redone lerps stand alone (the same code, integer taps 0..65535).  Under a clip box intersect_box takes the bounds per
 * axis in the oracle's operations; for the unit cube it is vo_intersect_box itself.  Build with -ffp-contract=off: every fused
 * operation is written. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vokselis_oracle.h"

/* flags per pixel, for the conditions the CPU fuzz asserts on the case list */
enum { GR_BOX = 1, GR_HIT = 2, GR_FIRST = 4, GR_NAN_SEEN = 8, GR_PINF_HIT = 16 };
enum { FMT_R8 = 0, FMT_R16F = 1, FMT_R16U = 3 };

typedef struct {
    const void *vol;
    uint32_t nx, ny, nz;
    int format;
} volume_t;

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

/* rec: the pixel's two float4 */
static int pixel(const vo_camera_uniform *cam, const volume_t *V, uint32_t W, uint32_t H, uint32_t x, uint32_t y, float dt_scale, float iso_k,
                 uint32_t refine, const float *box, float *rec, uint32_t *steps, float *a_out, uint32_t *flags) {
    float eye[3], dir[3], th[2];
    int bad = 0;
    vo_ray_naive(cam, W, H, x, y, eye, dir);
    intersect(eye, dir, box, th);
    *steps = 0;
    *a_out = 0.0f;
    *flags = 0;
    for (int k = 0; k < 8; k++) rec[k] = 0.0f;
    rec[3] = INFINITY; /* the miss record */
    if (th[0] > th[1]) return 0;
    *flags |= GR_BOX;
    th[0] = th[0] > 0.0f ? th[0] : 0.0f;
    const float dtx = 1.0f / ((float)V->nx * fabsf(dir[0])), dty = 1.0f / ((float)V->ny * fabsf(dir[1])), dtz = 1.0f / ((float)V->nz * fabsf(dir[2]));
    const float dt = dt_scale * fminf(dtx, fminf(dty, dtz));
    float p[3] = {eye[0] + th[0] * dir[0], eye[1] + th[0] * dir[1], eye[2] + th[0] * dir[2]};
    const float s[3] = {dir[0] * dt, dir[1] * dt, dir[2] * dt};
    int hit = 0;
    uint32_t it = 0, j = 0;
    for (float t = th[0]; t < th[1]; t = t + dt) {
        const float v = sample_at(V, p, NULL, &bad);
        it++;
        if (v != v) *flags |= GR_NAN_SEEN;
        if (v >= iso_k) {
            hit = 1;
            if (v == INFINITY) *flags |= GR_PINF_HIT;
            break;
        }
        p[0] = p[0] + s[0]; p[1] = p[1] + s[1]; p[2] = p[2] + s[2];
        j = j + 1;
    }
    *steps = it;
    if (bad) return -2;
    if (!hit) return 0;
    *flags |= GR_HIT;
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
        *flags |= GR_FIRST;
    }
    *a_out = a;
    const float q[3] = {fmaf(-a, s[0], p[0]), fmaf(-a, s[1], p[1]), fmaf(-a, s[2], p[2])};
    float g[3];
    const float xq = sample_at(V, q, g, &bad);
    if (bad) return -2;
    const float ex = q[0] - eye[0], ey = q[1] - eye[1], ez = q[2] - eye[2];
    const float mx = ex * dir[0];
    const float t = fmaf(ez, dir[2], fmaf(ey, dir[1], mx));
    rec[0] = q[0]; rec[1] = q[1]; rec[2] = q[2]; rec[3] = t;
    rec[4] = g[0]; rec[5] = g[1]; rec[6] = g[2]; rec[7] = xq;
    return 0;
}

/* The tile [tx, tx + tw) x [ty, ty + th) of a W x H frame (the origin may be negative: the part inside the frame is rendered).  format: 0
 * R8, 1 R16F, 3 R16_UNORM; iso_k on the kernel's scale; box: lo3, hi3 or NULL.  Outputs [H][W] (rec: [H][W][2][4] f32): steps (the
 * ray's iterations), a (the refined distance back), flags (above).  Pixels outside the tile are left as they are.  Returns 0, or -2 (see
 * sample_at). */
int geomr_render(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H,
                 int32_t tx, int32_t ty, uint32_t tw, uint32_t th, float dt_scale, float iso_k, uint32_t refine, const float *box,
                 float *out_rec, uint32_t *out_steps, float *out_a, uint32_t *out_flags) {
    const volume_t V = {vol, nx, ny, nz, format};
    const int64_t x1 = (int64_t)tx + tw, y1 = (int64_t)ty + th;
    for (int64_t y = ty < 0 ? 0 : ty; y < y1 && y < (int64_t)H; y++)
        for (int64_t x = tx < 0 ? 0 : tx; x < x1 && x < (int64_t)W; x++) {
            const size_t q = (size_t)y * W + (size_t)x;
            const int rc = pixel(cam, &V, W, H, (uint32_t)x, (uint32_t)y, dt_scale, iso_k, refine, box, out_rec + 8 * q, out_steps + q, out_a + q, out_flags + q);
            if (rc) return rc;
        }
    return 0;
}
