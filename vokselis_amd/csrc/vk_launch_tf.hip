// vk_launch_tf.hip -- the cell march under a runtime transfer function (vk_set_transfer_function): raymarch_naive_body (vk_march.hpp)
// with TF = true, for the layouts that carry a table -- LINEAR (u8, f16), PACKED (u8, f16), PACKED_PAIRS (u8) -- with and without
// skipping, both address paths, both output formats, with and without COUNT.  The skip walks take the loop (WALK_LOOP) and no
// probe-ahead: VK_RENDER_FAST_WALK is refused with a table (dispatch_march).
// The table is read with plain global loads (two 16-byte entries per sample, a 4 KiB table that stays in the L1 / L2): an LDS copy
// would cost every 64-lane block 4 KiB more LDS on top of the ~3 KiB of index tables.
#include "vk_ctx.hpp"
#include "vk_march.hpp"

using namespace vk;

template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_tf_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = true, LIT = false;  // (lit: vk_launch_lit.hip)
    const TfDesc *tfd = &T;
    const LightDesc *ldp = nullptr;
#include "vk_march_kernel_body.hpp"
}

template <int VOL, bool SKIP, bool SAFE>
static void launch_tf(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const TfDesc &T, uint32_t grid, bool count) {
    const bool f16 = ctx->out_format == VK_OUT_RGBA16F;
    VolumeDesc V = V_in;
    if (!SKIP && V.lut) V.lut += cell_lut_entries(V.nx, V.ny, V.nz);  // byte-offset copy of the tables (as launch_naive)
    constexpr bool lut = (VOL == VOL_P8 || VOL == VOL_P16 || VOL == VOL_PF16) && !SAFE;
    const uint32_t lds = (lut ? cell_lut_bytes(V.nx, V.ny, V.nz) : 0u) + ctx->naive_lds_pad;
    if (f16) {
        if (count) hipLaunchKernelGGL((raymarch_tf_kernel<VOL, SKIP, SAFE, OUT_RGBA16F, true>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T);
        else hipLaunchKernelGGL((raymarch_tf_kernel<VOL, SKIP, SAFE, OUT_RGBA16F, false>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T);
    } else {
        if (count) hipLaunchKernelGGL((raymarch_tf_kernel<VOL, SKIP, SAFE, OUT_RGBA32F, true>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T);
        else hipLaunchKernelGGL((raymarch_tf_kernel<VOL, SKIP, SAFE, OUT_RGBA32F, false>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T);
    }
}

template <int VOL>
static void launch_tf_packed(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, const TfDesc &T, uint32_t grid, bool count, bool skip, bool safe) {
    if (skip) { if (safe) launch_tf<VOL, true, true>(ctx, L, V, T, grid, count); else launch_tf<VOL, true, false>(ctx, L, V, T, grid, count); }
    else { if (safe) launch_tf<VOL, false, true>(ctx, L, V, T, grid, count); else launch_tf<VOL, false, false>(ctx, L, V, T, grid, count); }
}

// The caller (dispatch_march) has refused the layouts without table kernels.
void launch_cells_tf(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, const TfDesc &T, uint32_t grid, bool count, bool skip, bool safe) {
    switch (ctx->vol_kind) {
        case VOL_P8: launch_tf_packed<VOL_P8>(ctx, L, V, T, grid, count, skip, safe); break;
        case VOL_P16: launch_tf_packed<VOL_P16>(ctx, L, V, T, grid, count, skip, safe); break;
        case VOL_PF16: launch_tf_packed<VOL_PF16>(ctx, L, V, T, grid, count, skip, safe); break;
        case VOL_LINEAR_F16: launch_tf<VOL_LINEAR_F16, false, true>(ctx, L, V, T, grid, count); break;
        default: launch_tf<VOL_LINEAR_U8, false, true>(ctx, L, V, T, grid, count); break;
    }
}
