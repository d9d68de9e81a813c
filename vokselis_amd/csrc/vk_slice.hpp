// vk_slice.hpp -- the slice pass (vk_render_slice, vk_slice_probe): the descriptor the slice kernels read, a pixel's
// position on the plane, the inside test, the offset of a slab sample, the three reductions' steps, the validation of a caller's
// vk_slice (which also forms rn and the window's k1 / k2) and the arithmetic of the value surface's read-back, shared by the kernels
// (vk_launch_slice.hip), the host (vk_render.hip, vk_context.hip) and the host fuzz (tests/slice_fuzz.cpp, plain g++ under ASan / UBSan).
//
// A pixel's value record is two f32, 8 bytes: (x, 1) for a pixel whose position lies in the box -- x the filtered sample, or the slab's
// reduction, on the kernel's scale -- and (+0, 0) for every other pixel of the tile.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vokselis_hip.h"
#include "vk_tf.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VK_SLICE_HD __host__ __device__ __forceinline__
#else
#define VK_SLICE_HD inline
#endif

namespace vk {

constexpr size_t kSliceRecordBytes = 8;  // two f32 per pixel

// What the slice kernels read beside the volume: the plane, the slab, the box, the window of the table in force, the surfaces and the
// part of the tile that lies on the backbuffer.  Wave-uniform: kernel arguments, read by scalar loads.
struct SliceDesc {
    float origin[3]; float rn;    // rn = (float)(1.0 / (double)samples)
    float du[3]; float k1;        // k1, k2, umax, imax: tf_constants() of the table in force (the grey ramp without one)
    float dv[3]; float k2;
    float dn[3]; float umax;
    float lo[3]; int32_t imax;    // [lo, hi]: the clip box, or the unit cube
    float hi[3]; uint32_t samples;
    const float *rgba;            // the table's entries; nullptr: the grey ramp
    void *out;                    // the backbuffer, [H][W] pixels
    void *values;                 // the value surface, [H][W] records; nullptr without VK_SLICE_VALUES
    uint32_t W, H;
    uint32_t x0, y0, x1, y1;      // the tile on the backbuffer: pixels [x0, x1) x [y0, y1), 8x8 blocks from (x0, y0)
    int32_t reduce;
    uint32_t pad[3];
};
static_assert(sizeof(SliceDesc) == 160, "SliceDesc is read with scalar loads: a multiple of 16 bytes");

// P.c of backbuffer pixel (px, py): fma((float)py, dv.c, fma((float)px, du.c, origin.c)).  The conversions are exact (a backbuffer has far
// fewer than 2^24 pixels a side).
VK_SLICE_HD float slice_position(float origin, float du, float dv, uint32_t px, uint32_t py) { return fmaf((float)py, dv, fmaf((float)px, du, origin)); }

// lo.c <= P.c <= hi.c on all three axes; a NaN compares false: outside
VK_SLICE_HD bool slice_inside(float x, float y, float z, const float lo[3], const float hi[3]) {
    return lo[0] <= x && x <= hi[0] && lo[1] <= y && y <= hi[1] && lo[2] <= z && z <= hi[2];
}

// w of slab sample k: (float)k - 0.5f * (float)(samples - 1).  Exact: k and samples - 1 are at most 255, the product a multiple of 0.5.
VK_SLICE_HD float slab_offset(uint32_t k, uint32_t samples) { return (float)k - 0.5f * (float)(samples - 1u); }

// One step of a reduction, in the order of k.  A NaN sample compares false and is passed over; MAX starts at -inf, MIN at +inf, MEAN at +0.
VK_SLICE_HD float slab_max_step(float M, float x) { return x > M ? x : M; }
VK_SLICE_HD float slab_min_step(float M, float x) { return x < M ? x : M; }
VK_SLICE_HD float slab_mean_step(float acc, float x) { return acc + x; }

// A caller's slice into the descriptor's plane, slab and window.  Returns nullptr, or what is wrong (VK_ERR_INVALID).  tf_n: the entries of the
// table in force, 0: none -- the grey ramp, two entries over [0, 1].  dn is read (and held to the bounds) under samples > 1 only.
inline const char *slice_validate(const vk_slice *s, uint32_t tf_n, float tf_lo, float tf_hi, SampleScale scale, SliceDesc &D) {
    if (!s) return "slice is NULL";
    auto ok = [](const float v[3]) {
        for (int i = 0; i < 3; i++)
            if (!isfinite(v[i]) || fabsf(v[i]) > VK_SLICE_MAX_COORD) return false;
        return true;
    };
    if (!ok(s->origin) || !ok(s->du) || !ok(s->dv)) return "a component of origin, du or dv is not finite or beyond +-VK_SLICE_MAX_COORD";
    if (s->samples < 1u || s->samples > (uint32_t)VK_SLICE_MAX_SAMPLES) return "samples must be in [1, VK_SLICE_MAX_SAMPLES]";
    if (s->samples > 1u) {
        if (!ok(s->dn)) return "a component of dn is not finite or beyond +-VK_SLICE_MAX_COORD";
        if (s->reduce != VK_SLAB_MAX && s->reduce != VK_SLAB_MIN && s->reduce != VK_SLAB_MEAN) return "unknown reduce (VK_SLAB_MAX, VK_SLAB_MIN, VK_SLAB_MEAN)";
    }
    for (int i = 0; i < 3; i++) {
        D.origin[i] = s->origin[i]; D.du[i] = s->du[i]; D.dv[i] = s->dv[i];
        D.dn[i] = s->samples > 1u ? s->dn[i] : 0.0f;
    }
    D.samples = s->samples;
    D.reduce = s->samples > 1u ? s->reduce : (int32_t)VK_SLAB_MAX;
    D.rn = (float)(1.0 / (double)s->samples);
    const uint32_t n = tf_n ? tf_n : 2u;
    tf_constants(n, tf_n ? tf_lo : 0.0f, tf_n ? tf_hi : 1.0f, scale, D.k1, D.k2);
    D.umax = (float)(n - 1u);
    D.imax = (int32_t)n - 2;
    return nullptr;
}

// The value surface and its read-back: bytes of a row, of the surface, of the destination a read-back with `pitch` writes (its last
// row ends with the row, not the pitch), and the byte offset of pixel (x, y)'s record in either.
VK_SLICE_HD size_t slice_row_bytes(uint32_t width) { return (size_t)width * kSliceRecordBytes; }
VK_SLICE_HD size_t slice_surface_bytes(uint32_t width, uint32_t height) { return slice_row_bytes(width) * height; }
VK_SLICE_HD bool slice_pitch_ok(uint32_t width, size_t pitch) { return pitch >= slice_row_bytes(width); }
VK_SLICE_HD size_t slice_dst_bytes(uint32_t width, uint32_t height, size_t pitch) { return height == 0 ? 0 : pitch * (height - 1u) + slice_row_bytes(width); }
VK_SLICE_HD size_t slice_record_offset(uint32_t x, uint32_t y, size_t pitch) { return (size_t)y * pitch + (size_t)x * kSliceRecordBytes; }

// The part of the tile [tx, tx + tw) x [ty, ty + th) that lies on a W x H backbuffer: false when none does.
inline bool slice_tile_clip(int32_t tx, int32_t ty, uint32_t tw, uint32_t th, uint32_t W, uint32_t H, uint32_t &x0, uint32_t &y0, uint32_t &x1, uint32_t &y1) {
    const int64_t ax = tx < 0 ? 0 : (int64_t)tx, ay = ty < 0 ? 0 : (int64_t)ty;
    int64_t bx = (int64_t)tx + (int64_t)tw, by = (int64_t)ty + (int64_t)th;
    bx = bx > (int64_t)W ? (int64_t)W : bx;
    by = by > (int64_t)H ? (int64_t)H : by;
    if (bx <= ax || by <= ay) return false;
    x0 = (uint32_t)ax; y0 = (uint32_t)ay; x1 = (uint32_t)bx; y1 = (uint32_t)by;
    return true;
}

}  // namespace vk
