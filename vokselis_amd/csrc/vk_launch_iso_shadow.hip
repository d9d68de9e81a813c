// vk_launch_iso_shadow.hip -- the first-hit isosurface march with light-direction shadows (vk_set_shadows): the
// kernel body of vk_march_kernel_body.hpp with ISO = true and SHADOW = true.  Everything up to the shade is raymarch_iso_kernel's
// (vk_launch_iso.hip); in the epilogue a ray that hit marches once more, from its refined crossing along the light direction
// (vk_march_iso.hpp: iso_shadowed), and a shadowed point keeps 1 - strength of its diffuse and specular terms (vk_light.hpp).  Kernels of
// their own, launched only for a lit isosurface whose light is not a headlight, so that every render that does not shadow runs the code
// it ran before.  Same coverage as raymarch_iso_kernel: LINEAR (u8, f16), PACKED (u8, f16), PACKED_PAIRS (u8), with and without
// skipping, both address paths, both output formats, with and without COUNT; each with a twin under a clip box.
#include "vk_launch.hpp"
#include "vk_march.hpp"

using namespace vk;

static_assert(kernargs_fit<IsoDesc, ShadowDesc, ClipDesc>, "raymarch_iso_shadow_kernel, raymarch_iso_shadow_clip_kernel: LaunchDesc + VolumeDesc + IsoDesc + ShadowDesc (+ ClipDesc)");

template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_iso_shadow_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I, const ShadowDesc Sh) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = false, LIT = false, MIP = false, ISO = true;
    const TfDesc *tfd = nullptr;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = &I;
    constexpr bool CLIP = false;
    const ClipDesc *clp = nullptr;
    constexpr bool SHADOW = true;
    const ShadowDesc *shd = &Sh;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

// ... and under a clip box: the primary ray and the shadow ray march the same box.
template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_iso_shadow_clip_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I, const ShadowDesc Sh, const ClipDesc Cl) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = false, LIT = false, MIP = false, ISO = true;
    const TfDesc *tfd = nullptr;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = &I;
    constexpr bool CLIP = true;
    const ClipDesc *clp = &Cl;
    constexpr bool SHADOW = true;
    const ShadowDesc *shd = &Sh;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

// The caller (dispatch_march) has refused the layouts without isosurface kernels and chosen this family: lit, not a headlight.
void launch_cells_iso_shadow(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const IsoDesc &I, const ShadowDesc &Sh, const ClipDesc *Cl, uint32_t grid, bool count, bool skip,
                             bool safe) {
    auto launch = [&](auto CLIP) {
        with_table_layout(ctx, skip, safe, [&](auto VOL, auto SKIP, auto SAFE) {
            VolumeDesc V = V_in;
            const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
            with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
                if constexpr (CLIP()) hipLaunchKernelGGL((raymarch_iso_shadow_clip_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I, Sh, *Cl);
                else hipLaunchKernelGGL((raymarch_iso_shadow_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I, Sh);
            });
        });
    };
    if (!Cl) launch(bool_tag<false>()); else launch(bool_tag<true>());
}
