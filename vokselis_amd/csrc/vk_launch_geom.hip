// vk_launch_geom.hip -- the geometry pass of the first-hit isosurface (vk_render_geometry, vk_pick): the kernel body
// of vk_march_kernel_body.hpp with ISO = true and GEOM = true.  The frame, the ray, the loops (vk_march_iso.hpp) and the bisection are the
// isosurface colour kernels' (vk_launch_iso.hip); the epilogue refines whether or not lighting is set and stores the crossing, its distance
// along the ray, the gradient and the sample there (vk_geom.hpp) into the geometry surface instead of a colour into the backbuffer.
// Coverage is the isosurface family's: LINEAR (u8, f16), PACKED (u8, f16), PACKED_PAIRS (u8), with and without skipping, both address
// paths.  One output format and no COUNT: the pass writes neither the step image nor the counters.
// Each kernel has a twin under a clip box (vk_set_clip_box): raymarch_geom_clip_kernel, below.
#include "vk_launch.hpp"
#include "vk_march.hpp"

using namespace vk;

template <int VOL, bool SKIP, bool SAFE>
__global__ __launch_bounds__(64) void raymarch_geom_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I, const GeomDesc G) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr int OUT = OUT_RGBA32F;  // (unused: the pass stores no colour)
    constexpr bool COUNT = false;
    constexpr bool TF = false, LIT = false, MIP = false, ISO = true;
    const TfDesc *tfd = nullptr;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = &I;
    constexpr bool CLIP = false;
    const ClipDesc *clp = nullptr;
    constexpr bool SHADOW = false;
    const ShadowDesc *shd = nullptr;
    constexpr bool GEOM = true;
    const GeomDesc *gmd = &G;
#include "vk_march_kernel_body.hpp"
}

template <int VOL, bool SKIP, bool SAFE>
__global__ __launch_bounds__(64) void raymarch_geom_clip_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I, const GeomDesc G, const ClipDesc Cl) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr int OUT = OUT_RGBA32F;
    constexpr bool COUNT = false;
    constexpr bool TF = false, LIT = false, MIP = false, ISO = true;
    const TfDesc *tfd = nullptr;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = &I;
    constexpr bool CLIP = true;
    const ClipDesc *clp = &Cl;
    constexpr bool SHADOW = false;
    const ShadowDesc *shd = nullptr;
    constexpr bool GEOM = true;
    const GeomDesc *gmd = &G;
#include "vk_march_kernel_body.hpp"
}

// The caller (dispatch_march) has refused the layouts without isosurface kernels.
void launch_cells_geom(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const IsoDesc &I, const GeomDesc &G, const ClipDesc *Cl, uint32_t grid, bool skip, bool safe) {
    auto launch = [&](auto CLIP) {
        with_table_layout(ctx, skip, safe, [&](auto VOL, auto SKIP, auto SAFE) {
            VolumeDesc V = V_in;
            const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
            if constexpr (CLIP()) hipLaunchKernelGGL((raymarch_geom_clip_kernel<VOL(), SKIP(), SAFE()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I, G, *Cl);
            else hipLaunchKernelGGL((raymarch_geom_kernel<VOL(), SKIP(), SAFE()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I, G);
        });
    };
    if (!Cl) launch(bool_tag<false>()); else launch(bool_tag<true>());
}
