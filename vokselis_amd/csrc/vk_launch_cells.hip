// vk_launch_cells.hip -- instantiates raymarch_naive_kernel (vk_march.hpp) for every cell / comparison layout.
#include "vk_launch.hpp"
#include "vk_march.hpp"

using namespace vk;

template <int VOL, bool SKIP, bool SAFE, int WALK = WALK_LOOP, bool AHEAD = false>
static void launch_naive(vk_ctx *ctx, const LaunchDesc &L, VolumeDesc V, uint32_t grid, bool count) {
    const uint32_t lds = cell_kernel_lds<VOL, SKIP, SAFE, !AHEAD>(ctx, V);
    with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
        hipLaunchKernelGGL((raymarch_naive_kernel<VOL, SKIP, SAFE, WALK, AHEAD, OUT(), COUNT()>), dim3(grid), dim3(64), lds, ctx->stream, L, V);
    });
}

template <int VOL>
static void launch_packed(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, uint32_t grid, bool count, bool skip, bool safe, int walk) {
    // the probe-ahead trip (LF_PROBE_AHEAD: single-frame launches) exists for the skip kernels' fast path, unbounded march only
    const bool ahead = skip && !safe && (L.flags & LF_PROBE_AHEAD) && !(L.flags & LF_ADAPTIVE_PROBING);
    if (skip && walk == WALK_FMA) {
        if (safe) launch_naive<VOL, true, true, WALK_FMA>(ctx, L, V, grid, count);
        else if (ahead) launch_naive<VOL, true, false, WALK_FMA, true>(ctx, L, V, grid, count);
        else launch_naive<VOL, true, false, WALK_FMA>(ctx, L, V, grid, count);
    } else if (skip) {
        if (safe) launch_naive<VOL, true, true>(ctx, L, V, grid, count);
        else if (ahead) launch_naive<VOL, true, false, WALK_LOOP, true>(ctx, L, V, grid, count);
        else launch_naive<VOL, true, false>(ctx, L, V, grid, count);
    } else { if (safe) launch_naive<VOL, false, true>(ctx, L, V, grid, count); else launch_naive<VOL, false, false>(ctx, L, V, grid, count); }
}

void launch_cells(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, uint32_t grid, bool count, bool skip, bool safe, int walk) {
    switch (ctx->vol_kind) {
        case VOL_P8: launch_packed<VOL_P8>(ctx, L, V, grid, count, skip, safe, walk); break;
        case VOL_P16: launch_packed<VOL_P16>(ctx, L, V, grid, count, skip, safe, walk); break;
        case VOL_PF16: launch_packed<VOL_PF16>(ctx, L, V, grid, count, skip, safe, walk); break;
        case VOL_B9U8: launch_naive<VOL_B9U8, false, true>(ctx, L, V, grid, count); break;
        case VOL_B9F16: launch_naive<VOL_B9F16, false, true>(ctx, L, V, grid, count); break;
        case VOL_Q8: launch_naive<VOL_Q8, false, true>(ctx, L, V, grid, count); break;
        case VOL_QF16: launch_naive<VOL_QF16, false, true>(ctx, L, V, grid, count); break;
        case VOL_LINEAR_F16: launch_naive<VOL_LINEAR_F16, false, true>(ctx, L, V, grid, count); break;
        default: launch_naive<VOL_LINEAR_U8, false, true>(ctx, L, V, grid, count); break;
    }
}
