// vk_launch_compute.hip -- instantiates the compute twin (raycast_compute.wgsl) and the C3 procedural march (vk_compute.hpp).
#include "vk_launch.hpp"
#include "vk_compute.hpp"

using namespace vk;

void launch_procedural(vk_ctx *ctx, const LaunchDesc &L, uint32_t grid, bool count, float time, bool device_sine) {
    if (device_sine) {  // (tolerance mode: no counting instantiation of its own -- the counters describe the specified march)
        with_out(ctx, [&](auto OUT) { hipLaunchKernelGGL((raymarch_procedural_kernel<OUT(), false, true>), dim3(grid), dim3(64), 0, ctx->stream, L, time); });
        return;
    }
    with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
        hipLaunchKernelGGL((raymarch_procedural_kernel<OUT(), COUNT()>), dim3(grid), dim3(64), 0, ctx->stream, L, time);
    });
}

template <bool SKIP, int RING, int REV = 1>
static void launch_records(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, uint32_t grid, bool count) {
    const uint32_t lds = pair_lut_entries(V.nx, V.ny, V.nz) * 4u;
    with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
        hipLaunchKernelGGL((raymarch_compute_records_kernel<OUT(), COUNT(), SKIP, RING, REV>), dim3(grid), dim3(64), lds, ctx->stream, L, V);
    });
}

void launch_compute(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, uint32_t grid, bool count, bool records, bool skip) {
    if (records) {
        // request buffers x revolutions of the ring per loop iteration (vk_compute.hpp; profiles/r04_compute_twin_skip_and_ring.txt): a launch of
        // one frame that does not fill the machine (720p: 14 400 waves) is its longest waves' chains and gains from the deeper ring; launches
        // that do (1080p: 32 400; several frames) from the longer loop body
        // ... and a frame of a crowded ring of frames in flight (three executing) from the smallest ring: the xor 720p frame 0.0500 -> 0.0456 ms
        // per frame at k = 4 with four buffers and one revolution (6: 0.0500, 4 x 2: 0.0502; on one stream 4 costs 1.5 %)
        const uint32_t ring = ctx->pair_ring ? ctx->pair_ring : (frames_crowded(ctx) ? 4u : ((L.n_frames > 1 || L.n_blocks >= 24000u) ? 42u : 6u));
        if (!skip) launch_records<false, 4, 1>(ctx, L, V, grid, count);
        else if (ring == 42) launch_records<true, 4, 2>(ctx, L, V, grid, count);
        else if (ring == 6) launch_records<true, 6, 1>(ctx, L, V, grid, count);
        else launch_records<true, 4, 1>(ctx, L, V, grid, count);
        return;
    }
    with_out_count(ctx, count, [&](auto OUT, auto COUNT) {
        hipLaunchKernelGGL((raymarch_compute_kernel<OUT(), COUNT()>), dim3(grid), dim3(64), 0, ctx->stream, L, V);
    });
}
