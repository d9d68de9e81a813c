// vk_light.hpp -- gradient lighting of the table march (vk_set_lighting): the descriptor the lit kernels read, the analytic gradient of
// the trilinear interpolant and the shade of a sample, shared by the kernels (vk_launch_lit.hip), the host validation (vk_render.hip) and
// the host fuzz (tests/lit_fuzz.cpp, plain g++ under ASan / UBSan).
//
// Per sampled step, from the cell's taps t0..t7 (bit 0 = x, bit 1 = y, bit 2 = z) and the weights fx, fy, fz, with the sample's own
// c00, c10, c01, c11 (x-lerps) and l0, l1 (y-lerps), every operation one rounding, in this order:
//   dx00 = t1 - t0, dx10 = t3 - t2, dx01 = t5 - t4, dx11 = t7 - t6      (PACKED_PAIRS: the stored deltas, the same bits for u8 data)
//   gx = fma(fz, e1 - e0, e0),  e0 = fma(fy, dx10 - dx00, dx00),  e1 = fma(fy, dx11 - dx01, dx01)
//   gy = fma(fz, y1 - y0, y0),  y0 = c10 - c00,  y1 = c11 - c01
//   gz = l1 - l0
//   g = (gx * nx, gy * ny, gz * nz)                                     (world gradient: u = p n - 0.5)
//   q = fma(g.z, g.z, fma(g.y, g.y, g.x * g.x))
//   q finite and >= FLT_MIN:  N = g * rsqrt(q),  diff = |N.L|,  spec = |N.H|^shininess     (N.X = fma(N.z, X.z, fma(N.y, X.y, N.x * X.x)))
//   otherwise (no gradient: zero, subnormal, NaN or infinite):  diff = 1, spec = 0
//   rgb' = c.rgb * (ka + kd * diff) + ks * spec
// L is the unit light direction (the host normalises it in double and rounds each component once) or -dir for a headlight; V = -dir;
// H = (L + V) * (1 / sqrt(h.h)) once per ray (correctly rounded), or V when h.h < FLT_MIN.  The kernels take rsqrt, log2 and exp2 from
// the hardware (v_rsq, v_log, v_exp: ~1 ulp); the host forms here and the restatement (tests/lit_restatement.c) round correctly.
//
// Why skipping stays exact.  Lighting changes a sample's colour, never its alpha, so the trip counts, the early-out and the skip maps are
// those of the unlit table (vk_tf.hpp).  A skipped sample is one whose alpha is +0; sampled, it would add w * rgb' with w = (1 - A) * 0 = +0,
// which leaves every accumulator's bits as they are provided rgb' is finite.  It is: table colours are bounded by VK_TF_MAX_COLOUR (1e30),
// ka, kd, ks lie in [0, 16], diff is 1 or |N.L| <= ~1 (N and L unit vectors up to a few ulp), and spec = |N.H|^n <= (1 + 2^-20)^1024 < 1.001,
// so |rgb'| <= 1e30 * (16 + 16 * 1.001) + 16 * 1.001, far below FLT_MAX.  NaN or infinite taps take the no-gradient branch: the lighting
// factors stay finite whatever the taps (and such a cell is never empty: vk_tf.hpp).
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#include <initializer_list>

#if defined(__HIPCC__)
#define VK_LIGHT_HD __host__ __device__ __forceinline__
#else
#define VK_LIGHT_HD inline
#endif

namespace vk {

constexpr float kLightMaxK = 16.0f;                                // ka, kd, ks in [0, 16]
constexpr float kLightMinShininess = 1.0f, kLightMaxShininess = 1024.0f;

// What the lit kernels read (a kernel argument of their own): the unit light direction (unused with a headlight) and the coefficients.
struct LightDesc {
    float lx, ly, lz;
    int32_t headlight;
    float ka, kd, ks, shininess;
};
static_assert(sizeof(LightDesc) == 32, "LightDesc mirrors vk_lighting");

// Host validation of the public parameters (vk_lighting's fields, in order); fills the descriptor and returns nullptr, or returns what is wrong.
inline const char *light_desc(const float dir[3], int32_t headlight, float ka, float kd, float ks, float shininess, LightDesc &D) {
    for (float v : {dir[0], dir[1], dir[2], ka, kd, ks, shininess})
        if (!isfinite(v)) return "a field is not finite";
    if (!(ka >= 0.0f && ka <= kLightMaxK && kd >= 0.0f && kd <= kLightMaxK && ks >= 0.0f && ks <= kLightMaxK)) return "ambient, diffuse and specular must lie in [0, 16]";
    if (!(shininess >= kLightMinShininess && shininess <= kLightMaxShininess)) return "shininess must lie in [1, 1024]";
    D.headlight = headlight != 0;
    D.lx = D.ly = D.lz = 0.0f;
    if (!D.headlight) {
        const double x = dir[0], y = dir[1], z = dir[2], len = sqrt(x * x + y * y + z * z);
        if (!(len > 0.0)) return "the light direction is zero-length (set headlight for a light at the eye)";
        D.lx = (float)(x / len); D.ly = (float)(y / len); D.lz = (float)(z / len);
    }
    D.ka = ka; D.kd = kd; D.ks = ks; D.shininess = shininess;
    return nullptr;
}

// A ray's light constants: L (the light, or V for a headlight) and the half vector H, from the ray's unit direction.
struct LitRay {
    float lx, ly, lz, hx, hy, hz;
};

VK_LIGHT_HD LitRay lit_ray(const LightDesc &D, const float dir[3]) {
    const float vx = -dir[0], vy = -dir[1], vz = -dir[2];
    LitRay r;
    r.lx = D.headlight ? vx : D.lx; r.ly = D.headlight ? vy : D.ly; r.lz = D.headlight ? vz : D.lz;
    const float hx = r.lx + vx, hy = r.ly + vy, hz = r.lz + vz;
    const float q = fmaf(hz, hz, fmaf(hy, hy, hx * hx));
    if (q >= FLT_MIN) {
        const float s = 1.0f / sqrtf(q);
        r.hx = hx * s; r.hy = hy * s; r.hz = hz * s;
    } else {
        r.hx = vx; r.hy = vy; r.hz = vz;
    }
    return r;
}

// The sample's world gradient from the x-differences, the x-lerps and the y-lerps (the order of the header comment).
VK_LIGHT_HD void lit_gradient(float dx00, float dx10, float dx01, float dx11, float c00, float c10, float c01, float c11, float l0, float l1,
                              float fy, float fz, float nx, float ny, float nz, float &gx, float &gy, float &gz) {
    const float e0 = fmaf(fy, dx10 - dx00, dx00), e1 = fmaf(fy, dx11 - dx01, dx01);
    const float y0 = c10 - c00, y1 = c11 - c01;
    gx = fmaf(fz, e1 - e0, e0) * nx;
    gy = fmaf(fz, y1 - y0, y0) * ny;
    gz = (l1 - l0) * nz;
}

// rgb' of a sample of table colour (cr, cg, cb) with world gradient g.
VK_LIGHT_HD void lit_shade(const LightDesc &D, const LitRay &R, float gx, float gy, float gz, float &cr, float &cg, float &cb) {
    const float q = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
    const bool has = q >= FLT_MIN && q <= FLT_MAX;  // (false for NaN)
#if defined(__HIP_DEVICE_COMPILE__)
    const float s = __builtin_amdgcn_rsqf(has ? q : 1.0f);
#else
    const float s = 1.0f / sqrtf(has ? q : 1.0f);
#endif
    const float Nx = gx * s, Ny = gy * s, Nz = gz * s;
    const float nl = fabsf(fmaf(Nz, R.lz, fmaf(Ny, R.ly, Nx * R.lx)));
    const float nh = fabsf(fmaf(Nz, R.hz, fmaf(Ny, R.hy, Nx * R.hx)));
#if defined(__HIP_DEVICE_COMPILE__)
    const float p = __builtin_amdgcn_exp2f(D.shininess * __builtin_amdgcn_logf(nh));  // |N.H|^n; 0 -> log2 = -inf -> 0
#else
    const float p = (float)pow((double)nh, (double)D.shininess);
#endif
    const float diff = has ? nl : 1.0f, spec = has ? p : 0.0f;
    const float f = D.ka + D.kd * diff, sp = D.ks * spec;
    cr = cr * f + sp; cg = cg * f + sp; cb = cb * f + sp;
}

// ... and with the shadow factor k on the diffuse and specular terms (vk_set_shadows; vk_shadow.hpp): rgb' = c.rgb * (ka + kd * diff * k) +
// ks * spec * k, k = 1 - strength for a shadowed point and 1 otherwise.  A function of its own: the callers above keep their code.
VK_LIGHT_HD void lit_shade(const LightDesc &D, const LitRay &R, float gx, float gy, float gz, float k, float &cr, float &cg, float &cb) {
    const float q = fmaf(gz, gz, fmaf(gy, gy, gx * gx));
    const bool has = q >= FLT_MIN && q <= FLT_MAX;
#if defined(__HIP_DEVICE_COMPILE__)
    const float s = __builtin_amdgcn_rsqf(has ? q : 1.0f);
#else
    const float s = 1.0f / sqrtf(has ? q : 1.0f);
#endif
    const float Nx = gx * s, Ny = gy * s, Nz = gz * s;
    const float nl = fabsf(fmaf(Nz, R.lz, fmaf(Ny, R.ly, Nx * R.lx)));
    const float nh = fabsf(fmaf(Nz, R.hz, fmaf(Ny, R.hy, Nx * R.hx)));
#if defined(__HIP_DEVICE_COMPILE__)
    const float p = __builtin_amdgcn_exp2f(D.shininess * __builtin_amdgcn_logf(nh));
#else
    const float p = (float)pow((double)nh, (double)D.shininess);
#endif
    const float diff = has ? nl : 1.0f, spec = has ? p : 0.0f;
    const float f = D.ka + (D.kd * diff) * k, sp = (D.ks * spec) * k;
    cr = cr * f + sp; cg = cg * f + sp; cb = cb * f + sp;
}

}  // namespace vk
