// vk_launch_u16_geom.hip -- the geometry pass of the first-hit isosurface (vk_render_geometry) on R16_UNORM volumes:
// the family beside U16_ISO (vk_launch_u16_iso.hip), LINEAR and PACKED, every variant, with and without a clip box.  A kernel template
// of its own: raymarch_u16_kernel (vk_march_u16.hpp) keeps its signature and its device code.
#include "vk_march_u16.hpp"

using namespace vk;

template <int VOL, bool SKIP, bool SAFE>
__global__ __launch_bounds__(64) void raymarch_u16_geom_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I, const GeomDesc G) {
    static_assert(is_u16_kind(VOL), "the R16_UNORM layouts");
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
__global__ __launch_bounds__(64) void raymarch_u16_geom_clip_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I, const GeomDesc G, const ClipDesc Cl) {
    static_assert(is_u16_kind(VOL), "the R16_UNORM layouts");
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

// The caller (dispatch_march) has checked that the volume is an R16_UNORM one.
void launch_u16_geom(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const IsoDesc &I, const GeomDesc &G, const ClipDesc *Cl, uint32_t grid, bool skip, bool safe) {
    auto variants = [&](auto CLIP, auto VOL, auto SKIP, auto SAFE) {
        VolumeDesc V = V_in;
        const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
        if constexpr (CLIP()) hipLaunchKernelGGL((raymarch_u16_geom_clip_kernel<VOL(), SKIP(), SAFE()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I, G, *Cl);
        else hipLaunchKernelGGL((raymarch_u16_geom_kernel<VOL(), SKIP(), SAFE()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I, G);
    };
    auto layouts = [&](auto CLIP) {
        if (ctx->vol_kind == VOL_PU16) with_skip_safe(skip, safe, [&](auto SKIP, auto SAFE) { variants(CLIP, int_tag<VOL_PU16>(), SKIP, SAFE); });
        else variants(CLIP, int_tag<VOL_LINEAR_U16>(), bool_tag<false>(), bool_tag<true>());
    };
    if (Cl) layouts(bool_tag<true>()); else layouts(bool_tag<false>());
}
