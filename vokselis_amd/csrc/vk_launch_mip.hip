// vk_launch_mip.hip -- the cell march under the maximum-intensity projection (vk_set_projection(VK_PROJ_MAX)):
// the kernel body of vk_march_kernel_body.hpp with MIP = true.  The frame is the other families': block and pixel mapping, cull, index
// tables, ray set-up, probing policy, counters and trace.  The projection's own: the loops (vk_march_mip.hpp: another operator on the
// filtered sample, U = mip_update(U, x), the running maximum in table coordinates) and the body's epilogue under MIP (the table looked up
// once per ray).  Same coverage as the table kernels (vk_launch_tf.hip): LINEAR (u8, f16), PACKED (u8, f16), PACKED_PAIRS (u8), with and
// without skipping, both address paths, both output formats, with and without COUNT; the skip walks take the loop (WALK_LOOP), no
// probe-ahead, no trip log.
// Each kernel has a twin under a clip box (vk_set_clip_box): raymarch_mip_clip_kernel, below.
#include "vk_launch.hpp"
#include "vk_march.hpp"

using namespace vk;

// T: the window of the table in force; T.rgba == nullptr: the implicit grey ramp.
template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_mip_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = false, LIT = false, MIP = true, ISO = false;
    const TfDesc *tfd = &T;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = nullptr;
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
__global__ __launch_bounds__(64) void raymarch_mip_clip_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T, const ClipDesc Cl) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = false, LIT = false, MIP = true, ISO = false;
    const TfDesc *tfd = &T;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = nullptr;
    constexpr bool CLIP = true;
    const ClipDesc *clp = &Cl;
    constexpr bool SHADOW = false;
    const ShadowDesc *shd = nullptr;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

// The caller (dispatch_march) has refused the layouts without MIP kernels.
void launch_cells_mip(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const TfDesc &T, const ClipDesc *Cl, uint32_t grid, bool count, bool skip, bool safe) {
    // (the kernels without a box first: they stay where they were in the unit's device code)
    auto launch = [&](auto CLIP) {
        with_table_layout(ctx, skip, safe, [&](auto VOL, auto SKIP, auto SAFE) {
            VolumeDesc V = V_in;
            const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
            with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
                if constexpr (CLIP()) hipLaunchKernelGGL((raymarch_mip_clip_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, *Cl);
                else hipLaunchKernelGGL((raymarch_mip_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T);
            });
        });
    };
    if (!Cl) launch(bool_tag<false>()); else launch(bool_tag<true>());
}
