// vk_launch_u16_iso_shadow.hip -- the first-hit isosurface march with light-direction shadows (vk_set_shadows) on
// R16_UNORM volumes: the family beside U16_ISO (vk_launch_u16_iso.hip), LINEAR and PACKED, every variant, with and without a clip box.
// A kernel template of its own: raymarch_u16_kernel (vk_march_u16.hpp) keeps its signature and its device code.
#include "vk_march_u16.hpp"

using namespace vk;

static_assert(kernargs_fit<IsoDesc, ShadowDesc, ClipDesc>, "raymarch_u16_iso_shadow_kernel: LaunchDesc + VolumeDesc + IsoDesc + ShadowDesc + ClipDesc");

template <bool CLIPPED, int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_u16_iso_shadow_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I, const ShadowDesc Sh, const ClipDesc Cl) {
    static_assert(is_u16_kind(VOL), "the R16_UNORM layouts");
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = false, LIT = false, MIP = false, ISO = true;
    const TfDesc *tfd = nullptr;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = &I;
    constexpr bool CLIP = CLIPPED;
    const ClipDesc *clp = &Cl;
    constexpr bool SHADOW = true;
    const ShadowDesc *shd = &Sh;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

// The caller (dispatch_march) has checked that the volume is an R16_UNORM one and chosen this family: lit, not a headlight.
void launch_u16_iso_shadow(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const IsoDesc &I, const ShadowDesc &Sh, const ClipDesc *Cl, uint32_t grid, bool count, bool skip,
                           bool safe) {
    auto variants = [&](auto CLIP, auto VOL, auto SKIP, auto SAFE) {
        VolumeDesc V = V_in;
        const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
        const ClipDesc box = Cl ? *Cl : ClipDesc{};
        with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
            hipLaunchKernelGGL((raymarch_u16_iso_shadow_kernel<CLIP(), VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I, Sh, box);
        });
    };
    auto layouts = [&](auto CLIP) {
        if (ctx->vol_kind == VOL_PU16) with_skip_safe(skip, safe, [&](auto SKIP, auto SAFE) { variants(CLIP, int_tag<VOL_PU16>(), SKIP, SAFE); });
        else variants(CLIP, int_tag<VOL_LINEAR_U16>(), bool_tag<false>(), bool_tag<true>());
    };
    if (Cl) layouts(bool_tag<true>()); else layouts(bool_tag<false>());
}
