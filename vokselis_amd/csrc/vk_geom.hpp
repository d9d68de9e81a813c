// vk_geom.hpp -- the geometry pass of the first-hit isosurface (vk_render_geometry, vk_pick): the descriptor the
// geometry kernels read, the record they write, the distance along the ray, the flags the pass accepts and the arithmetic of the
// geometry surface's read-back, shared by the kernels (vk_launch_geom.hip, vk_launch_u16_geom.hip through vk_march_kernel_body.hpp), the
// host (vk_render.hip, vk_context.hip) and the host fuzz (tests/geom_fuzz.cpp, plain g++ under ASan / UBSan).
//
// A pixel's record is two float4, 32 bytes: { (q.x, q.y, q.z, t), (g.x, g.y, g.z, x) } for a ray that hit -- q = fma(-a, s, p) per component
// with a the isosurface's bisection (vk_iso.hpp; run whether or not lighting is set), t the distance of q along the unit ray, g the
// gradient of vk_light.hpp's lit_gradient at q on the kernel's scale, not normalised, x the filtered sample at q -- and the miss record
// { (0, 0, 0, +inf), (0, 0, 0, 0) } for every other pixel of the tile.  isfinite(t) is the hit mask.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/vokselis_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VK_GEOM_HD __host__ __device__ __forceinline__
#else
#define VK_GEOM_HD inline
#endif

namespace vk {

constexpr size_t kGeomRecordBytes = 32;  // two float4 per pixel

// What the geometry kernels read beside the isosurface's arguments: the geometry surface, [H][W][2] float4.
struct GeomDesc {
    void *surface;
    uint32_t pad[2];
};
static_assert(sizeof(GeomDesc) == 16, "GeomDesc is read with scalar loads: 16 bytes");

// The miss record's words: (0, 0, 0, +inf), (0, 0, 0, 0).
constexpr uint32_t kGeomMissBits[8] = {0u, 0u, 0u, 0x7f800000u, 0u, 0u, 0u, 0u};

// The distance of q along the unit ray from the eye, one rounding per operation: fma(q.z - e.z, d.z, fma(q.y - e.y, d.y, (q.x - e.x) * d.x)).
VK_GEOM_HD float geom_distance(float qx, float qy, float qz, const float eye[3], const float dir[3]) {
    const float dx = qx - eye[0], dy = qy - eye[1], dz = qz - eye[2];
    const float m = dx * dir[0];
    return fmaf(dz, dir[2], fmaf(dy, dir[1], m));
}

// The flags vk_render_geometry takes: the colour render's skip policy, nothing else.  Returns nullptr, or what is wrong; *unsupported
// says whether that is VK_ERR_UNSUPPORTED (a flag the isosurface family has no kernels for) or VK_ERR_INVALID (any other flag).
constexpr uint32_t kGeomFlags = VK_RENDER_NO_SKIP | VK_RENDER_SAFE | VK_RENDER_FORCE_SKIP | VK_RENDER_PROBE_ALWAYS;
inline const char *geom_flags_check(uint32_t flags, bool *unsupported) {
    *unsupported = false;
    if (flags & ~(kGeomFlags | (uint32_t)VK_RENDER_FAST_WALK))
        return "vk_render_geometry: takes VK_RENDER_NO_SKIP, VK_RENDER_SAFE, VK_RENDER_FORCE_SKIP and VK_RENDER_PROBE_ALWAYS only";
    if (flags & VK_RENDER_FAST_WALK) {
        *unsupported = true;
        return "isosurface: VK_RENDER_FAST_WALK has no isosurface kernels";
    }
    return nullptr;
}

// The geometry surface and its read-back: bytes of a row, of the surface, of the destination a read-back with `pitch` writes (its last
// row ends with the row, not the pitch), and the byte offset of pixel (x, y)'s record in either.
VK_GEOM_HD size_t geom_row_bytes(uint32_t width) { return (size_t)width * kGeomRecordBytes; }
VK_GEOM_HD size_t geom_surface_bytes(uint32_t width, uint32_t height) { return geom_row_bytes(width) * height; }
VK_GEOM_HD bool geom_pitch_ok(uint32_t width, size_t pitch) { return pitch >= geom_row_bytes(width); }
VK_GEOM_HD size_t geom_dst_bytes(uint32_t width, uint32_t height, size_t pitch) { return height == 0 ? 0 : pitch * (height - 1u) + geom_row_bytes(width); }
VK_GEOM_HD size_t geom_record_offset(uint32_t x, uint32_t y, size_t pitch) { return (size_t)y * pitch + (size_t)x * kGeomRecordBytes; }

#if defined(__HIPCC__)
__device__ __forceinline__ float4 geom_miss0() { return make_float4(0.0f, 0.0f, 0.0f, __builtin_inff()); }
__device__ __forceinline__ float4 geom_miss1() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// A pixel's record: two 16-byte vector stores at the pixel's place in the [H][W][2] surface (x < W and y < H: the caller's pm.valid).
__device__ __forceinline__ void geom_store(const GeomDesc &G, uint32_t W, int32_t x, int32_t y, const float4 r0, const float4 r1) {
    float4 *rec = reinterpret_cast<float4 *>(G.surface) + ((size_t)(uint32_t)y * W + (size_t)(uint32_t)x) * 2u;
    rec[0] = r0;
    rec[1] = r1;
}

#endif

}  // namespace vk
