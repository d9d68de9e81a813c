// vk_launch_thick.hip -- local thickness of a value range (vk_local_thickness): for every voxel of S the largest
// capped D2 among the centres whose open ball holds it.  The request's validation, the cap, the reach, the box distances and the two
// skips are vk_thick.hpp's, shared with the host fuzz; the distance kernels (vk_dist_launch.hpp) are borrowed as they are.
//
//   distance   D2(not S, .): the distance pass's first round.
//   tile max   the largest Dc of each tile of 8^3 voxels, one word per tile.
//   thickness  a gather by output tile: a workgroup owns a tile, a thread a voxel and its running T2, which starts at Dc(v).  The
//              workgroup walks the source tiles within reach -- its own first --, skips those thick_tile_skipped tells it to, loads an
//              accepted tile's 512 Dc, keeps the centres thick_centre_kept passes by ballot compaction into an LDS list, and every
//              thread takes the maximum over the list.  A tile without foreground, or whose foreground starts at C, walks nothing.
//   stats      the four totals as one set of partial results per workgroup.
//   dense      one kernel per texel class: sqrtf(T2) * gain through the fill rule, or the fill; the host forms the automatic gain
//              from the stats before it.
// Phases are separated by kernel boundaries: no workgroup waits for another, no address is written by two threads of a launch, there
// are no global atomics and no float atomics.  Every loop has a bound: the grid-stride loops their item count, the walk the window's
// tiles (at most kThickMaxWindow^3), the list its length (at most 512, in steps of kThickListStep).  Every barrier stands in a loop whose trip count and branches
// depend on block-uniform values alone: the tile numbers, the tile maxima, the box distances and `lowest`, which every thread reads from
// LDS behind a barrier.  Plain C++; no inline assembly; the one per-thread array is the four list entries of a trip, unrolled into registers (ScratchSize 0).
#include "vk_dist_launch.hpp"
#include "vk_label.hpp"
#include "vk_pass_blocks.hpp"
#include "vk_texel.hpp"
#include "vk_thick.hpp"

using namespace vk;

constexpr uint32_t kThickWaves = kThickThreads / 64u;
constexpr uint32_t kThickListStep = 4;  // list entries per trip: their LDS loads are issued together, ahead of the arithmetic
constexpr uint32_t kThickVoxelThreads = 256, kThickStatsWords = 4, kThickNone = 0xffffffffu;

struct ThickDesc {
    uint32_t nx, ny, nz, ntx, nty, ntz;
    uint32_t tiles, cap;       // cap: C
    uint32_t w[3], reach[3];   // reach: thick_reach per axis
    uint64_t n;
    uint32_t fill_bits;
    float gain;
};
static_assert(sizeof(ThickDesc) % 8 == 0 && pass_kernargs_fit<ThickDesc>, "thickness kernels: ThickDesc");

// Dc of voxel (lx, ly, lz) of the tile whose box is b, or 0 where the tile's box ends before it.  a: D2(not S, .), 0 off S.
__device__ __forceinline__ uint32_t thick_load_dc(const ThickDesc &T, const ThickBox &b, uint32_t lx, uint32_t ly, uint32_t lz, const uint32_t *__restrict__ a, uint64_t &i) {
    const uint32_t x = b.lo[0] + lx, y = b.lo[1] + ly, z = b.lo[2] + lz;
    if (x > b.hi[0] || y > b.hi[1] || z > b.hi[2]) { i = 0u; return 0u; }
    i = voxel_index(x, y, z, T.nx, T.ny);
    const uint32_t d = a[i];
    return d < T.cap ? d : T.cap;
}

__global__ __launch_bounds__(kThickThreads) void thick_tile_max_kernel(const ThickDesc T, const uint32_t *__restrict__ a, uint32_t *__restrict__ tile_max) {
    __shared__ uint32_t s_max;
    const uint32_t lx = threadIdx.x % kThickTile, ly = threadIdx.x / kThickTile % kThickTile, lz = threadIdx.x / (kThickTile * kThickTile);
    for (uint32_t t = blockIdx.x; t < T.tiles; t += gridDim.x) {  // block-uniform
        if (threadIdx.x == 0) s_max = 0u;
        __syncthreads();
        uint32_t tx, ty, tz;
        tile_coords(t, T.ntx, T.nty, tx, ty, tz);
        uint64_t i;
        const uint32_t top = wave_reduce(thick_load_dc(T, thick_tile_box(tx, ty, tz, T.nx, T.ny, T.nz), lx, ly, lz, a, i), WaveMax());
        if ((threadIdx.x & (warpSize - 1)) == 0 && top) atomicMax(&s_max, top);
        __syncthreads();
        if (threadIdx.x == 0) tile_max[t] = s_max;
        __syncthreads();  // the next tile's reset
    }
}

// t2[v] = T2(v) over the whole volume.  a: D2(not S, .); tile_max: thick_tile_max_kernel's.
__global__ __launch_bounds__(kThickThreads) void thick_gather_kernel(const ThickDesc T, const uint32_t *__restrict__ a, const uint32_t *__restrict__ tile_max, uint32_t *__restrict__ t2) {
    __shared__ uint4 s_list[kThickTileVoxels + kThickListStep];  // a kept centre: its position w_c u_c per axis, and its Dc; padded to whole steps with Dc = 0, which raises nothing
    __shared__ uint32_t s_count[kThickWaves];
    __shared__ uint32_t s_low;
    const uint32_t lx = threadIdx.x % kThickTile, ly = threadIdx.x / kThickTile % kThickTile, lz = threadIdx.x / (kThickTile * kThickTile);
    const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
    for (uint32_t t = blockIdx.x; t < T.tiles; t += gridDim.x) {  // block-uniform
        uint32_t tx, ty, tz;
        tile_coords(t, T.ntx, T.nty, tx, ty, tz);
        const ThickBox out = thick_tile_box(tx, ty, tz, T.nx, T.ny, T.nz);
        uint64_t at;
        uint32_t best = thick_load_dc(T, out, lx, ly, lz, a, at);
        const bool inside = out.lo[0] + lx <= out.hi[0] && out.lo[1] + ly <= out.hi[1] && out.lo[2] + lz <= out.hi[2];
        const bool fg = best != 0u;  // Dc > 0 exactly on S
        const int32_t qx = (int32_t)(T.w[0] * (out.lo[0] + lx)), qy = (int32_t)(T.w[1] * (out.lo[1] + ly)), qz = (int32_t)(T.w[2] * (out.lo[2] + lz));

        if (threadIdx.x == 0) s_low = kThickNone;
        __syncthreads();
        {
            const uint32_t low = wave_reduce(fg ? best : kThickNone, WaveMin());
            if (lane == 0u && low != kThickNone) atomicMin(&s_low, low);
        }
        __syncthreads();
        uint32_t lowest = s_low;  // the smallest running T2 of the tile's foreground; kThickNone: there is none
        __syncthreads();           // ... read by everyone before the walk resets it

        if (lowest != kThickNone && lowest < T.cap) {  // block-uniform
            uint32_t fx, gx, fy, gy, fz, gz;
            thick_window(tx, T.ntx, T.reach[0], fx, gx);
            thick_window(ty, T.nty, T.reach[1], fy, gy);
            thick_window(tz, T.ntz, T.reach[2], fz, gz);
            const uint32_t wx = gx - fx + 1u, wy = gy - fy + 1u, wz = gz - fz + 1u, steps = wx * wy * wz;
            for (uint32_t j = 0; j <= steps && lowest < T.cap; j++) {  // block-uniform: step 0 is the tile itself
                uint32_t sx = tx, sy = ty, sz = tz;
                if (j > 0u) {
                    const uint32_t k = j - 1u, row = k / wx;
                    sx = fx + (k - row * wx);
                    sz = fz + row / wy;
                    sy = fy + (row - (row / wy) * wy);
                    if (sx == tx && sy == ty && sz == tz) continue;
                }
                const uint32_t top = tile_max[thick_tile_index(sx, sy, sz, T.ntx, T.nty)];
                const ThickBox src = thick_tile_box(sx, sy, sz, T.nx, T.ny, T.nz);
                if (thick_tile_skipped(top, thick_box_box_d2(src, out, T.w), lowest)) continue;

                uint64_t i;
                const uint32_t dc = thick_load_dc(T, src, lx, ly, lz, a, i);
                const uint32_t ux = src.lo[0] + lx, uy = src.lo[1] + ly, uz = src.lo[2] + lz;
                const bool keep = dc != 0u && thick_centre_kept(dc, thick_voxel_box_d2(ux, uy, uz, out, T.w), lowest);
                const unsigned long long mask = __ballot(keep);
                if (lane == 0u) s_count[wave] = (uint32_t)__popcll(mask);
                __syncthreads();
                uint32_t base = 0u, total = 0u;
                for (uint32_t k = 0; k < kThickWaves; k++) {
                    const uint32_t c = s_count[k];
                    base += k < wave ? c : 0u;
                    total += c;
                }
                if (keep) s_list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = make_uint4(T.w[0] * ux, T.w[1] * uy, T.w[2] * uz, dc);
                if (threadIdx.x < kThickListStep) s_list[total + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
                if (threadIdx.x == 0) s_low = kThickNone;
                __syncthreads();
                for (uint32_t k = 0; k < total; k += kThickListStep) {
                    uint4 c[kThickListStep];
#pragma unroll
                    for (uint32_t e = 0; e < kThickListStep; e++) c[e] = s_list[k + e];
#pragma unroll
                    for (uint32_t e = 0; e < kThickListStep; e++) {
                        const uint32_t d2 = thick_d2((int32_t)c[e].x, (int32_t)c[e].y, (int32_t)c[e].z, qx, qy, qz);
                        best = (d2 < c[e].w && c[e].w > best) ? c[e].w : best;
                    }
                }
                {
                    const uint32_t low = wave_reduce(fg ? best : kThickNone, WaveMin());
                    if (lane == 0u) atomicMin(&s_low, low);
                }
                __syncthreads();
                lowest = s_low;
                __syncthreads();  // ... before the next tile's counts, list and reset
            }
        }
        if (inside) t2[at] = fg ? best : 0u;
    }
}

// partial[4 b + ...]: |S|, the voxels at C, the sum of T2 and the largest T2 over workgroup b's voxels
__global__ __launch_bounds__(kThickVoxelThreads) void thick_stats_kernel(const ThickDesc T, const uint32_t *__restrict__ t2, unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n[kThickStatsWords];
    __shared__ uint32_t s_max;
    if (threadIdx.x < kThickStatsWords) s_n[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) s_max = 0u;
    __syncthreads();
    unsigned long long n_fg = 0ull, n_sat = 0ull, sum = 0ull;
    uint32_t top = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * kThickVoxelThreads + threadIdx.x; i < T.n; i += (uint64_t)gridDim.x * kThickVoxelThreads) {
        const uint32_t v = t2[i];
        n_fg += v != 0u; n_sat += v == T.cap; sum += v;
        top = v > top ? v : top;
    }
    block_add(&s_n[0], n_fg); block_add(&s_n[1], n_sat); block_add(&s_n[2], sum);
    top = wave_reduce(top, WaveMax());
    if ((threadIdx.x & (warpSize - 1)) == 0 && top) atomicMax(&s_max, top);
    __syncthreads();
    if (threadIdx.x == 0) s_n[3] = s_max;
    publish_partials<kThickStatsWords>(partial, s_n);
}

template <int CLASS>
__global__ __launch_bounds__(kThickVoxelThreads) void thick_dense_kernel(const ThickDesc T, const uint32_t *__restrict__ t2, void *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThickVoxelThreads + threadIdx.x; i < T.n; i += (uint64_t)gridDim.x * kThickVoxelThreads) {
        const uint32_t v = t2[i];
        uint32_t bits = T.fill_bits;
        if (v != 0u) {
            const float root = sqrtf((float)v);  // T2 <= 2^22: the conversion is exact
            const float w = root * T.gain;
            bits = store_gained_bits<CLASS>(w);
        }
        store_texel_bits<CLASS>(out, i, bits);
    }
}

extern "C" {

int vk_local_thickness(vk_ctx *ctx, const vk_thickness_request *req, const vk_voxel_box *box, uint32_t *t2_out, void *dense_out, vk_thickness_result *result) {
    static const char *const entry = "vk_local_thickness";
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = thick_validate(req, t2_out != nullptr, dense_out != nullptr, result != nullptr)) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + why);
    const bool install = (req->flags & VK_THICK_INSTALL) != 0u;
    if (int rc = pass_install_refused(ctx, entry, "VK_THICK_INSTALL", install)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, entry, "thickness")) return rc;
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, entry, "VK_THICK_CLIP_BOX", box, (req->flags & VK_THICK_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, entry, "thickness")) return rc;
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    if (n > kDistMaxVoxels) return fail(ctx, VK_ERR_UNSUPPORTED, "thickness: a volume of more than 2^32 - 2 voxels (voxel indices are 32-bit)");
    if (!dist_d2_fits(req->spacing, ctx->nx, ctx->ny, ctx->nz))
        return fail(ctx, VK_ERR_UNSUPPORTED, "thickness: sum_c (spacing[c] (n_c - 1))^2 exceeds 0xFFFFFFFE: a squared distance would not fit in 32 bits");

    const float lo_k = label_scale_bound(req->lo, ctx->format), hi_k = label_scale_bound(req->hi, ctx->format);
    ThickDesc T{};
    T.nx = ctx->nx; T.ny = ctx->ny; T.nz = ctx->nz;
    T.ntx = thick_tiles_along(ctx->nx); T.nty = thick_tiles_along(ctx->ny); T.ntz = thick_tiles_along(ctx->nz);
    T.tiles = T.ntx * T.nty * T.ntz;  // <= n / 512 + ...: 32 bits hold it
    T.cap = (uint32_t)thick_cap(req->max_radius);
    for (int c = 0; c < 3; c++) { T.w[c] = req->spacing[c]; T.reach[c] = thick_reach(T.cap, req->spacing[c]); }
    T.n = n;
    T.fill_bits = label_fill_bits(req->fill_out, ctx->format);
    const uint32_t tile_blocks = label_blocks(T.tiles, ctx->thick_max_blocks);
    const uint32_t voxel_blocks = std::min<uint32_t>(label_blocks((n + kThickVoxelThreads - 1u) / kThickVoxelThreads, ctx->thick_max_blocks), kPassMaxPartials);  // a set of partial results per workgroup

    const int kind = ctx->vol_kind;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, entry};
    // (debug, vk_debug_set_param("thick_timing", k): phase k alone between the context's timer events, read with vk_timer_elapsed_ms --
    //  1 distance, 2 tile max, 3 thickness, 4 stats, 5 dense)
    const uint32_t timing = ctx->thick_timing;

    const size_t dense_bytes = pass_dense_bytes(ctx->format, n);
    DeviceTemp d_a, d_b, d_stack, d_tile_max, d_partial, d_out;
    if (int rc = call.alloc(d_a, (size_t)n * 4u, "the distance array")) return rc;
    if (int rc = call.alloc(d_b, (size_t)n * 4u, "the thickness array")) return rc;
    if (int rc = call.alloc(d_stack, (size_t)n * 4u, "the envelope stacks")) return rc;
    if (int rc = call.alloc(d_tile_max, (size_t)T.tiles * 4u, "the tile maxima")) return rc;
    PassPartials sums(voxel_blocks, kThickStatsWords);
    if (int rc = call.alloc(d_partial, sums.bytes(), "the partial totals")) return rc;
    if (dense_out || install)
        if (int rc = call.alloc(d_out, dense_bytes, "the output buffer")) return rc;
    uint32_t *a = (uint32_t *)d_a.p, *t2 = (uint32_t *)d_b.p, *tile_max = (uint32_t *)d_tile_max.p;
    unsigned long long *partial = (unsigned long long *)d_partial.p;

    // D2(not S, .) into a (b is its scratch), then T2 into b
    call.phase(timing == 1u, [&] { dist_launch_inside(ctx, B, lo_k, hi_k, req->spacing, a, t2, (uint32_t *)d_stack.p); });
    call.phase(timing == 2u, [&] { hipLaunchKernelGGL(thick_tile_max_kernel, dim3(tile_blocks), dim3(kThickThreads), 0, ctx->stream, T, (const uint32_t *)a, tile_max); });
    call.phase(timing == 3u, [&] { hipLaunchKernelGGL(thick_gather_kernel, dim3(tile_blocks), dim3(kThickThreads), 0, ctx->stream, T, (const uint32_t *)a, (const uint32_t *)tile_max, t2); });
    call.phase(timing == 4u, [&] { hipLaunchKernelGGL(thick_stats_kernel, dim3(voxel_blocks), dim3(kThickVoxelThreads), 0, ctx->stream, T, (const uint32_t *)t2, partial); });
    sums.download(call, partial);
    call.download(t2_out, t2, (size_t)n * 4u);
    if (int rc = call.finish()) return rc;

    vk_thickness_result r{};
    r.n_foreground = sums.sum(0u); r.n_saturated = sums.sum(1u); r.sum_t2 = sums.sum(2u);
    r.max_t2 = (uint32_t)sums.max(3u);
    r.gain = req->gain != 0.0f ? req->gain : thick_auto_gain(r.max_t2);
    T.gain = r.gain;
    if (dense_out || install) {
        call.phase(timing == 5u, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(thick_dense_kernel<texel_class(VOL())>, dim3(voxel_blocks), dim3(kThickVoxelThreads), 0, ctx->stream, T, (const uint32_t *)t2, d_out.p);
            });
        });
        call.download(dense_out, d_out.p, dense_bytes);
        if (int rc = call.finish()) return rc;
    }
    if (result) *result = r;
    return install ? call.install(d_out, T.nx, T.ny, T.nz, ctx->format, ctx->layout) : VK_OK;
}

}  // extern "C"
