// vk_launch_lit.hip -- the table march with gradient lighting (vk_set_lighting): raymarch_naive_body (vk_march.hpp) with TF = true and
// LIT = true, for the layouts that carry a table -- LINEAR (u8, f16), PACKED (u8, f16), PACKED_PAIRS (u8) -- with and without skipping,
// both address paths, both output formats, with and without COUNT, the skip walks taking the loop (as vk_launch_tf.hip).
// The shade reads only the sample's own taps (vk_light.hpp): no memory traffic beyond the table kernels', ALU work only.
#include "vk_ctx.hpp"
#include "vk_march.hpp"

using namespace vk;

template <int VOL, bool SKIP, bool SAFE, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_lit_kernel(const LaunchDesc L, const VolumeDesc V, const TfDesc T, const LightDesc Lt) {
    constexpr int WALK = WALK_LOOP;
    constexpr bool AHEAD = false;
    constexpr bool TF = true, LIT = true;
    const TfDesc *tfd = &T;
    const LightDesc *ldp = &Lt;
#include "vk_march_kernel_body.hpp"
}

template <int VOL, bool SKIP, bool SAFE>
static void launch_lit(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V_in, const TfDesc &T, const LightDesc &Lt, uint32_t grid, bool count) {
    const bool f16 = ctx->out_format == VK_OUT_RGBA16F;
    VolumeDesc V = V_in;
    if (!SKIP && V.lut) V.lut += cell_lut_entries(V.nx, V.ny, V.nz);  // byte-offset copy of the tables (as launch_naive)
    constexpr bool lut = (VOL == VOL_P8 || VOL == VOL_P16 || VOL == VOL_PF16) && !SAFE;
    const uint32_t lds = (lut ? cell_lut_bytes(V.nx, V.ny, V.nz) : 0u) + ctx->naive_lds_pad;
    if (f16) {
        if (count) hipLaunchKernelGGL((raymarch_lit_kernel<VOL, SKIP, SAFE, OUT_RGBA16F, true>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, Lt);
        else hipLaunchKernelGGL((raymarch_lit_kernel<VOL, SKIP, SAFE, OUT_RGBA16F, false>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, Lt);
    } else {
        if (count) hipLaunchKernelGGL((raymarch_lit_kernel<VOL, SKIP, SAFE, OUT_RGBA32F, true>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, Lt);
        else hipLaunchKernelGGL((raymarch_lit_kernel<VOL, SKIP, SAFE, OUT_RGBA32F, false>), dim3(grid), dim3(64), lds, ctx->stream, L, V, T, Lt);
    }
}

template <int VOL>
static void launch_lit_packed(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, const TfDesc &T, const LightDesc &Lt, uint32_t grid, bool count, bool skip, bool safe) {
    if (skip) { if (safe) launch_lit<VOL, true, true>(ctx, L, V, T, Lt, grid, count); else launch_lit<VOL, true, false>(ctx, L, V, T, Lt, grid, count); }
    else { if (safe) launch_lit<VOL, false, true>(ctx, L, V, T, Lt, grid, count); else launch_lit<VOL, false, false>(ctx, L, V, T, Lt, grid, count); }
}

// The caller (dispatch_march) has refused the layouts without table kernels, and lighting without a table.
void launch_cells_lit(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, const TfDesc &T, const LightDesc &Lt, uint32_t grid, bool count, bool skip, bool safe) {
    switch (ctx->vol_kind) {
        case VOL_P8: launch_lit_packed<VOL_P8>(ctx, L, V, T, Lt, grid, count, skip, safe); break;
        case VOL_P16: launch_lit_packed<VOL_P16>(ctx, L, V, T, Lt, grid, count, skip, safe); break;
        case VOL_PF16: launch_lit_packed<VOL_PF16>(ctx, L, V, T, Lt, grid, count, skip, safe); break;
        case VOL_LINEAR_F16: launch_lit<VOL_LINEAR_F16, false, true>(ctx, L, V, T, Lt, grid, count); break;
        default: launch_lit<VOL_LINEAR_U8, false, true>(ctx, L, V, T, Lt, grid, count); break;
    }
}
