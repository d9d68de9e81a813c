// vk_launch_tf.hip -- the cell march under a runtime transfer function (vk_set_transfer_function): raymarch_naive_body (vk_march.hpp)
// with TF = true, for the layouts that carry a table -- LINEAR (u8, f16), PACKED (u8, f16), PACKED_PAIRS (u8) -- with and without
// skipping, both address paths, both output formats, with and without COUNT.  The skip walks take the loop (WALK_LOOP) and no
// probe-ahead: VK_RENDER_FAST_WALK is refused with a table (dispatch_march).
// The table is read with plain global loads (two 16-byte entries per sample, a 4 KiB table that stays in the L1 / L2): an LDS copy
// would cost every 64-lane block 4 KiB more LDS on top of the ~3 KiB of index tables.
// Each kernel has a twin under a clip box (vk_set_clip_box): raymarch_tf_clip_kernel, below.
#include "vk_launch.hpp"
#include "vk_march.hpp"

using namespace vk;

template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_tf_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = true, LIT = false, MIP = false, ISO = false;  // (lit: vk_launch_lit.hip)
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
__global__ __launch_bounds__(64) void raymarch_tf_clip_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T, const ClipDesc Cl) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = true, LIT = false, MIP = false, ISO = false;  // (lit: vk_launch_lit.hip)
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

// The caller (dispatch_march) has refused the layouts without table kernels.
void launch_cells_tf(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const TfDesc &T, const ClipDesc *Cl, uint32_t grid, bool count, bool skip, bool safe) {
    // (the kernels without a box first: they stay where they were in the unit's device code)
    auto launch = [&](auto CLIP) {
        with_table_layout(ctx, skip, safe, [&](auto VOL, auto SKIP, auto SAFE) {
            VolumeDesc V = V_in;
            const uint32_t lds = cell_kernel_lds<VOL(), SKIP(), SAFE()>(ctx, V);
            with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
                if constexpr (CLIP()) hipLaunchKernelGGL((raymarch_tf_clip_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, *Cl);
                else hipLaunchKernelGGL((raymarch_tf_kernel<VOL(), SKIP(), SAFE(), OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T);
            });
        });
    };
    if (!Cl) launch(bool_tag<false>()); else launch(bool_tag<true>());
}
