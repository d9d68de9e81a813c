// vk_launch_slice.hip -- the slice pass (vk_render_slice, vk_slice_probe): a plane through the volume, windowed by the
// table in force, optionally a thick slab reduced by maximum, minimum or mean.  A kernel family of its own: no ray, no box intersection,
// no trip budget, no skip maps.  One lane per pixel, a 64-lane workgroup per 8x8 pixel block, so a wave's taps share cells and cache
// lines.  The sample is iso_sample() (vk_march_iso.hpp) -- the filter of every march, bit for bit -- through the clamped address path only
// (what SAFE is elsewhere): slab samples may leave the cube, and the saturating float-to-int conversion plus the index clamp keep every
// fetch inside the array; no index tables in LDS.  The value is mapped as the maximum projection maps its U (vk_tf.hpp: mip_update from
// +0, then the epilogue's lookup), put through sRGB and stored in the backbuffer's format; under VALUES the pixel's (x, weight) record goes
// to the value surface.  Coverage: LINEAR (u8, f16, u16), PACKED (u8, f16, u16), PACKED_PAIRS (u8); both output formats.
// samples == 1 and the three reductions are wave-uniform branches on kernel arguments: the choice stays on the scalar unit.
#include "vk_launch.hpp"
#include "vk_march.hpp"
#include "vk_slice.hpp"

using namespace vk;

static_assert(pass_kernargs_fit<SliceDesc>, "slice_kernel: VolumeDesc + SliceDesc");

template <int VOL>
__device__ __forceinline__ float slice_sample(const VolumeDesc &V, const float x, const float y, const float z) {
    return iso_sample<VOL, false, true>(V, nullptr, x, y, z).x;
}

// The slab: samples at P + w_k dn, reduced in the order of k.  The body takes two samples per iteration -- both positions, both fetches,
// then both steps -- so two samples' loads are in flight; a loop of one is a chain of dependent gathers.  An odd count ends with one.
template <int VOL, class Step>
__device__ __forceinline__ float slab_reduce(const VolumeDesc &V, const SliceDesc &S, const float Px, const float Py, const float Pz, float M, Step step) {
    const uint32_t n = S.samples;
    uint32_t k = 0;
#if defined(VK_EXP_SLICE_PLAIN_LOOP)  // (tools/variant.py: the loop of one sample per iteration, bitwise the same frames, for tools/slice_quick.py's A/B)
    for (; k < n; k++) {
        const float w0 = slab_offset(k, n);
        M = step(M, slice_sample<VOL>(V, fmaf(w0, S.dn[0], Px), fmaf(w0, S.dn[1], Py), fmaf(w0, S.dn[2], Pz)));
    }
#else
    for (; k + 1u < n; k += 2u) {
        const float w0 = slab_offset(k, n), w1 = slab_offset(k + 1u, n);
        const float a = slice_sample<VOL>(V, fmaf(w0, S.dn[0], Px), fmaf(w0, S.dn[1], Py), fmaf(w0, S.dn[2], Pz));
        const float b = slice_sample<VOL>(V, fmaf(w1, S.dn[0], Px), fmaf(w1, S.dn[1], Py), fmaf(w1, S.dn[2], Pz));
        M = step(M, a);
        M = step(M, b);
    }
    if (k < n) {
        const float w0 = slab_offset(k, n);
        M = step(M, slice_sample<VOL>(V, fmaf(w0, S.dn[0], Px), fmaf(w0, S.dn[1], Py), fmaf(w0, S.dn[2], Pz)));
    }
#endif
    return M;
}

template <int VOL, int OUT, bool VALUES>
__global__ __launch_bounds__(64) void slice_kernel(const VolumeDesc V, const SliceDesc S) {
    const uint32_t lane = threadIdx.x;
    const uint32_t px = S.x0 + blockIdx.x * 8u + (lane & 7u), py = S.y0 + blockIdx.y * 8u + (lane >> 3);
    if (px >= S.x1 || py >= S.y1) return;  // x1 <= W, y1 <= H (slice_tile_clip): every pixel below lies on the surfaces
    const size_t idx = (size_t)py * S.W + (size_t)px;
    const float Px = slice_position(S.origin[0], S.du[0], S.dv[0], px, py);
    const float Py = slice_position(S.origin[1], S.du[1], S.dv[1], px, py);
    const float Pz = slice_position(S.origin[2], S.du[2], S.dv[2], px, py);
    if (!slice_inside(Px, Py, Pz, S.lo, S.hi)) {  // the clear colour, like a miss
        store_pixel<OUT>(S.out, idx, 0.0f, 0.0f, 0.0f, 1.0f);
        if constexpr (VALUES) reinterpret_cast<float2 *>(S.values)[idx] = make_float2(0.0f, 0.0f);
        return;
    }
    float x;
    if (S.samples == 1u) x = slice_sample<VOL>(V, Px, Py, Pz);
    else if (S.reduce == VK_SLAB_MEAN) x = slab_reduce<VOL>(V, S, Px, Py, Pz, 0.0f, [](float a, float v) { return slab_mean_step(a, v); }) * S.rn;
    else if (S.reduce == VK_SLAB_MIN) x = slab_reduce<VOL>(V, S, Px, Py, Pz, __builtin_inff(), [](float m, float v) { return slab_min_step(m, v); });
    else x = slab_reduce<VOL>(V, S, Px, Py, Pz, -__builtin_inff(), [](float m, float v) { return slab_max_step(m, v); });
    // the maximum projection's value after one sample, and its epilogue's lookup (vk_march_kernel_body.hpp under MIP)
    const float U = mip_update(0.0f, x, S.k1, S.k2, S.umax);
    float cr = U, cg = U, cb = U;
    if (S.rgba) {
        const int i = tf_index(U, S.imax);
        const float f = U - (float)i;
        const float4 *E = reinterpret_cast<const float4 *>(S.rgba);
        const float4 e0 = E[i], e1 = E[i + 1];
        cr = fmaf(f, e1.x - e0.x, e0.x); cg = fmaf(f, e1.y - e0.y, e0.y); cb = fmaf(f, e1.z - e0.z, e0.z);
    }
    store_pixel<OUT>(S.out, idx, linear_to_srgb(cr), linear_to_srgb(cg), linear_to_srgb(cb), 1.0f);
    if constexpr (VALUES) reinterpret_cast<float2 *>(S.values)[idx] = make_float2(x, 1.0f);
}

// The caller (vk_render_slice) has refused the layouts without slice kernels and clipped the tile to the backbuffer.
void launch_slice(vk_ctx *ctx, const VolumeDesc &V, const SliceDesc &S) {
    const dim3 grid((S.x1 - S.x0 + 7u) / 8u, (S.y1 - S.y0 + 7u) / 8u);
    with_scalar_kind(ctx->vol_kind, [&](auto VOL) {
        with_out(ctx, [&](auto OUT) {
            if (S.values) hipLaunchKernelGGL((slice_kernel<VOL(), OUT(), true>), grid, dim3(64), 0, ctx->stream, V, S);
            else hipLaunchKernelGGL((slice_kernel<VOL(), OUT(), false>), grid, dim3(64), 0, ctx->stream, V, S);
        });
    });
}
