// vk_launch_iso.hip -- the cell march under first-hit isosurface rendering (vk_set_isosurface): the kernel body
// of vk_march_kernel_body.hpp with ISO = true.  The frame is the other families': block and pixel mapping, cull, index tables, ray
// set-up, probing policy, counters and trace.  The isosurface's own: the loops (vk_march_iso.hpp: one compare on the filtered sample,
// x >= iso_k, the hit sample's position kept) and the body's epilogue under ISO (the crossing refined by bisection and shaded once per
// ray, lighting a runtime branch: one family).  Same coverage as the table and MAX kernels: LINEAR (u8, f16), PACKED (u8, f16),
// PACKED_PAIRS (u8), with and without skipping, both address paths, both output formats, with and without COUNT; the skip walks take
// the loop (WALK_LOOP), no probe-ahead, no trip log.
// Each kernel has a twin under a clip box (vk_set_clip_box): raymarch_iso_clip_kernel, below.
#include "vk_launch.hpp"
#include "vk_march.hpp"

using namespace vk;

template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_iso_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = false, LIT = false, MIP = false, ISO = true;
    const TfDesc *tfd = nullptr;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = &I;
    constexpr bool CLIP = false;
    const ClipDesc *clp = nullptr;
    constexpr bool SHADOW = false;
    const ShadowDesc *shd = nullptr;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

// ... and under a clip box (vk_set_clip_box): the same body with CLIP = true and the box as a further argument.  Kernels of their own, so that the
// renders without a box run the code they ran before there was one.
template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_iso_clip_kernel(const LaunchDesc L, const VolumeDesc V, const IsoDesc I, const ClipDesc Cl) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = false, LIT = false, MIP = false, ISO = true;
    const TfDesc *tfd = nullptr;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = &I;
    constexpr bool CLIP = true;
    const ClipDesc *clp = &Cl;
    constexpr bool SHADOW = false;
    const ShadowDesc *shd = nullptr;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

// The caller (dispatch_march) has refused the layouts without isosurface kernels.
void launch_cells_iso(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const IsoDesc &I, const ClipDesc *Cl, uint32_t grid, bool count, bool skip, bool safe) {
    // (the kernels without a box first: they stay where they were in the unit's device code)
    auto launch = [&](auto CLIP) {
        with_table_layout(ctx, skip, safe, [&](auto VOL, auto SKIP, auto SAFE) {
            VolumeDesc V = V_in;
            const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
            with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
                if constexpr (CLIP()) hipLaunchKernelGGL((raymarch_iso_clip_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I, *Cl);
                else hipLaunchKernelGGL((raymarch_iso_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, I);
            });
        });
    };
    if (!Cl) launch(bool_tag<false>()); else launch(bool_tag<true>());
}
