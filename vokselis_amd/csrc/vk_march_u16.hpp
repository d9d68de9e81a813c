// vk_march_u16.hpp -- the cell march on R16_UNORM volumes (VK_FMT_R16_UNORM): one kernel template over the five
// NAIVE_TRILINEAR families -- built-in, table, lit, MAX, isosurface -- and their twins under a clip box, for the two layouts of the
// format: LINEAR (VOL_LINEAR_U16, 2 B per voxel) and PACKED (VOL_PU16: 16-byte cells of eight u16 taps in PF16's order, the same skip
// maps, index tables and fast-path bounds).  The body is vk_march_kernel_body.hpp, the loops are the other formats' (vk_march.hpp,
// vk_march_mip.hpp, vk_march_iso.hpp); what differs is the tap decode (vk_march_parts.hpp: xlerp_cell_dx, linear_taps) and the
// scale the host folds into the families' constants, S = 65535.  Every family takes the table family's variant set: with and without
// skipping, both address paths, both output formats, with and without COUNT; the walks take the loop (WALK_LOOP), no probe-ahead,
// no lone-speckle codes.  Each family is instantiated in a unit of its own (vk_launch_u16_*.hip), so the other formats' units keep
// their device code.
#pragma once

#include "vk_launch.hpp"
#include "vk_march.hpp"

namespace vk {

enum U16Family : int { U16_BUILTIN = 0, U16_TF = 1, U16_LIT = 2, U16_MIP = 3, U16_ISO = 4 };

static_assert(kernargs_fit<TfDesc, LightDesc, IsoDesc, ClipDesc>, "raymarch_u16_kernel: LaunchDesc + VolumeDesc + every family's descriptor");

// One signature for all families: a family reads its own descriptors (scalar loads from the kernel arguments) and never touches the others.
template <int FAM, bool CLIPPED, int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_u16_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T, const LightDesc Li, const IsoDesc I, const ClipDesc Cl) {
    static_assert(is_u16_kind(VOL), "the R16_UNORM layouts");
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = FAM == U16_TF || FAM == U16_LIT, LIT = FAM == U16_LIT, MIP = FAM == U16_MIP, ISO = FAM == U16_ISO;
    const TfDesc *tfd = &T;
    const LightDesc *ldp = &Li;
    const IsoDesc *isd = &I;
    constexpr bool CLIP = CLIPPED;
    const ClipDesc *clp = &Cl;
    constexpr bool SHADOW = false;
    const ShadowDesc *shd = nullptr;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

// The caller (dispatch_march) has checked that the volume is an R16_UNORM one.  Cl: nullptr for the kernels without a box (the built-in family has no others).
template <int FAM>
void launch_u16_family(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const TfDesc &T, const LightDesc &Li, const IsoDesc &I, const ClipDesc *Cl,
                       uint32_t grid, bool count, bool skip, bool safe) {
    auto variants = [&](auto CLIP, auto VOL, auto SKIP, auto SAFE) {
        VolumeDesc V = V_in;
        const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
        const ClipDesc box = Cl ? *Cl : ClipDesc{};
        with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
            hipLaunchKernelGGL((raymarch_u16_kernel<FAM, CLIP(), VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, Li, I, box);
        });
    };
    auto layouts = [&](auto CLIP) {
        if (ctx->vol_kind == VOL_PU16) with_skip_safe(skip, safe, [&](auto SKIP, auto SAFE) { variants(CLIP, int_tag<VOL_PU16>(), SKIP, SAFE); });
        else variants(CLIP, int_tag<VOL_LINEAR_U16>(), bool_tag<false>(), bool_tag<true>());
    };
    if constexpr (FAM != U16_BUILTIN) { if (Cl) { layouts(bool_tag<true>()); return; } }
    layouts(bool_tag<false>());
}

}  // namespace vk
