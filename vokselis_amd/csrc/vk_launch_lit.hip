// vk_launch_lit.hip -- the table march with gradient lighting (vk_set_lighting): raymarch_naive_body (vk_march.hpp) with TF = true and
// LIT = true, for the layouts that carry a table -- LINEAR (u8, f16), PACKED (u8, f16), PACKED_PAIRS (u8) -- with and without skipping,
// both address paths, both output formats, with and without COUNT, the skip walks taking the loop (as vk_launch_tf.hip).
// The shade reads only the sample's own taps (vk_light.hpp): no memory traffic beyond the table kernels', ALU work only.
// Each kernel has a twin under a clip box (vk_set_clip_box): raymarch_lit_clip_kernel, below.
#include "vk_launch.hpp"
#include "vk_march.hpp"

using namespace vk;

template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_lit_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T, const LightDesc Lt) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = true, LIT = true, MIP = false, ISO = false;
    const TfDesc *tfd = &T;
    const LightDesc *ldp = &Lt;
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
__global__ __launch_bounds__(64) void raymarch_lit_clip_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T, const LightDesc Lt, const ClipDesc Cl) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = true, LIT = true, MIP = false, ISO = false;
    const TfDesc *tfd = &T;
    const LightDesc *ldp = &Lt;
    const IsoDesc *isd = nullptr;
    constexpr bool CLIP = true;
    const ClipDesc *clp = &Cl;
    constexpr bool SHADOW = false;
    const ShadowDesc *shd = nullptr;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

// The caller (dispatch_march) has refused the layouts without table kernels, and lighting without a table.
void launch_cells_lit(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const TfDesc &T, const LightDesc &Lt, const ClipDesc *Cl, uint32_t grid, bool count, bool skip, bool safe) {
    // (the kernels without a box first: they stay where they were in the unit's device code)
    auto launch = [&](auto CLIP) {
        with_table_layout(ctx, skip, safe, [&](auto VOL, auto SKIP, auto SAFE) {
            VolumeDesc V = V_in;
            const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
            with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
                if constexpr (CLIP()) hipLaunchKernelGGL((raymarch_lit_clip_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, Lt, *Cl);
                else hipLaunchKernelGGL((raymarch_lit_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, Lt);
            });
        });
    };
    if (!Cl) launch(bool_tag<false>()); else launch(bool_tag<true>());
}
