// vk_launch_geo.hip -- geodesic distance through a value range (vk_geodesic_distance): for every voxel of S the
// length of the shortest path inside S from the source set, as exact integers.  The request's validation, the step costs, the saturating
// relaxation, the face predicate, a voxel's relaxation and the tile and halo arithmetic are vk_geo.hpp's, shared with the host fuzz.
//
//   seed    one kernel per volume kind, a workgroup per tile: the state word of every voxel (0 on the source set A, VK_GEO_INF
//           elsewhere), a foreground byte per voxel -- no later kernel touches the volume --, |S| and |A| as partial sums per workgroup,
//           and the mark of round 1 on every tile that holds a source or faces one across a tile border.
//   relax   the hot path, one launch per round, a workgroup per tile: a tile whose mark is not this round's is left at once.  An active
//           tile loads its state words and a one-voxel halo into LDS, relaxes its own voxels there in place until a whole pass lowers
//           nothing, stores the voxels it lowered and marks, for the next round, every neighbouring tile that a lowered voxel faces.
//   stats   the totals as one set of partial results per workgroup.
//   dense   one kernel per texel class: (float)g * gain through the fill rule, or one of the two fills; the host forms the automatic
//           gain from the stats before it.
// A voxel's word is written by the workgroup that owns its tile and by nobody else; another workgroup of the same launch may read it
// for its halo and see the value of before (every value a word holds is the length of a real path, words only
// decrease, and the owner marks the reader for the next launch, which sees the new value).  No workgroup waits for another: no spinning,
// no device-side queue, no persistent kernel; a round is a launch.
// The active set is one word per tile and parity of the round: round r runs the tiles whose word in array r & 1 equals r and writes
// r + 1 into array (r + 1) & 1.  A stamp needs no clearing between rounds and no compaction launch, several workgroups that wake the
// same tile store the same value, and a reader of array r & 1 never races a writer, which is in the other array; what it costs is one
// idle workgroup -- a scalar load and an exit -- per inactive tile and round.
// Every loop has a bound: the grid-stride loops their item count; the LDS passes the tile's foreground voxels + 1 (while the halo is
// fixed, every pass but the last settles at least the unsettled voxel of smallest final value: at most 4096 lowering passes and the one
// that finds nothing); the host's rounds end because every round that wakes a tile lowered a word, and words are non-negative integers.
// Every barrier stands where control flow is block-uniform: the tile number, the tile's mark (no workgroup of the launch writes the array
// it is read from) and the pass flag, which every thread reads from LDS behind a barrier.  Plain C++; no inline assembly.
// geo_relax_kernel's registers, LDS and occupancy, from hipcc -S for gfx950: the kernel's comment.
#include "vk_geo.hpp"
#include "vk_launch.hpp"
#include "vk_pass_blocks.hpp"
#include "vk_texel.hpp"

using namespace vk;

constexpr uint32_t kGeoVoxelThreads = 256, kGeoStatsWords = 6, kGeoSeedWords = 2;

struct GeoDesc {
    uint32_t nx, ny, nz, conn_sum;
    uint32_t ntx, nty, ntz, tiles;
    vk_voxel_box box;
    float lo_k, hi_k;
    uint32_t source_faces, target_faces, n_seeds, round;
    uint32_t fill_out_bits, fill_unreached_bits;
    float gain;
    uint32_t pad;
    uint64_t n;
    uint32_t seeds[VK_GEO_MAX_SEEDS];  // linear indices
    GeoWeights W;
    uint32_t pad2;
};
static_assert(sizeof(GeoDesc) % 8 == 0 && pass_kernargs_fit<GeoDesc>, "geodesic kernels: VolumeDesc + GeoDesc");

// the window in LDS, shared by the waves of a workgroup while they lower it: relaxed loads and stores of whole words
struct GeoLds {
    static __device__ __forceinline__ uint32_t load(const uint32_t *p, uint32_t i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ __forceinline__ void store(uint32_t *p, uint32_t i, uint32_t v) { __hip_atomic_store(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

// the directions of s_dirs, by the first 27 threads: the tiles that exist take `stamp`.  Returns, in thread 0, how many were marked.
__device__ __forceinline__ uint32_t geo_mark_tiles(const GeoDesc &G, uint32_t tx, uint32_t ty, uint32_t tz, uint32_t dirs, uint32_t *__restrict__ marks, uint32_t stamp) {
    bool marked = false;
    if (threadIdx.x < kLabelOffsets && ((dirs >> threadIdx.x) & 1u)) {
        uint32_t nb;
        if (geo_tile_neighbour(tx, ty, tz, G.ntx, G.nty, G.ntz, threadIdx.x, nb)) { marks[nb] = stamp; marked = true; }
    }
    return (uint32_t)__popcll(__ballot(marked));  // threads 0 .. 26 share wave 0
}

// state, fg: the whole volume.  marks: the array of round 1.  partial[2 b + ...]: |S| and |A| over workgroup b's tiles.
template <int VOL>
__global__ __launch_bounds__(kLabelThreads) void geo_seed_kernel(const VolumeDesc V, const GeoDesc G, uint32_t *__restrict__ state, uint8_t *__restrict__ fg, uint32_t *__restrict__ marks,
                                                                 unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n[kGeoSeedWords];
    __shared__ uint32_t s_dirs;
    if (threadIdx.x < kGeoSeedWords) s_n[threadIdx.x] = 0ull;
    uint32_t n_fg = 0u, n_src = 0u;
    for (uint32_t t = blockIdx.x; t < G.tiles; t += gridDim.x) {  // block-uniform
        if (threadIdx.x == 0) s_dirs = 0u;
        __syncthreads();
        uint32_t tx, ty, tz;
        tile_coords(t, G.ntx, G.nty, tx, ty, tz);
        const uint32_t x0 = tx * kLabelTile.tx, y0 = ty * kLabelTile.ty, z0 = tz * kLabelTile.tz;
        uint32_t dirs = 0u;
        for (uint32_t k = 0; k < kLabelPerThread; k++) {
            uint32_t lx, ly, lz;
            label_local_coords(threadIdx.x + k * kLabelThreads, lx, ly, lz);
            const uint32_t x = x0 + lx, y = y0 + ly, z = z0 + lz;
            if (x >= G.nx || y >= G.ny || z >= G.nz) continue;
            const uint32_t i = (uint32_t)voxel_index(x, y, z, G.nx, G.ny);
            const bool in_s = label_in_box(x, y, z, G.box) && label_foreground(texel_f32<VOL>(voxel_texel_bits<VOL>(V, x, y, z)), G.lo_k, G.hi_k);
            bool source = in_s && geo_on_faces(x, y, z, G.box, G.source_faces);
            for (uint32_t s = 0; s < G.n_seeds; s++) source = source || (in_s && G.seeds[s] == i);
            fg[i] = in_s ? 1u : 0u;
            state[i] = source ? 0u : kGeoInf;
            n_fg += in_s; n_src += source;
            if (source) dirs |= geo_wake_mask(lx, ly, lz, G.conn_sum) | (1u << kLabelCentre);
        }
        dirs = wave_reduce(dirs, WaveOr());
        if ((threadIdx.x & (warpSize - 1)) == 0 && dirs) atomicOr(&s_dirs, dirs);
        __syncthreads();
        (void)geo_mark_tiles(G, tx, ty, tz, s_dirs, marks, 1u);
        __syncthreads();  // the next tile's reset
    }
    block_add(&s_n[0], n_fg); block_add(&s_n[1], n_src);
    publish_partials<kGeoSeedWords>(partial, s_n);
}

// One round (G.round).  marks_cur: the tiles of this round; marks_next: those of the next.  counts[0 .. 4): the tiles this round woke,
// the tiles it visited, their LDS passes and the voxels it stored.
// CONN_SUM (1, 2, 3 for connectivity 6, 18, 26) is a template parameter: the neighbour set is known where geo_relax_voxel is unrolled,
// so a voxel's 6, 18 or 26 LDS loads are issued together instead of one behind a branch each.
// hipcc -S, gfx950, for <1>, <2>, <3>: 42, 51, 59 VGPRs, 82, 98, 106 SGPRs, none spilled to scratch (ScratchSize 0), 24496 bytes of
// LDS each.  LDS bounds the occupancy: 6 workgroups of 4 waves on a CU (160 KiB), 6 waves per SIMD; the registers would allow 8.
// A tile needs at most 4097 LDS passes per visit (above); a front that crosses a full tile along x takes 33, because the lanes of a
// wave hold consecutive x and read one another's words of the pass before.
template <uint32_t CONN_SUM>
__global__ __launch_bounds__(kLabelThreads) void geo_relax_kernel(const GeoDesc G, uint32_t *__restrict__ state, const uint8_t *__restrict__ fg, const uint32_t *__restrict__ marks_cur,
                                                                  uint32_t *__restrict__ marks_next, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t win[kGeoWindow];
    __shared__ uint32_t s_flag, s_dirs;
    __shared__ unsigned long long s_written;
    for (uint32_t t = blockIdx.x; t < G.tiles; t += gridDim.x) {  // block-uniform
        if (marks_cur[t] != G.round) continue;                     // block-uniform: nobody writes marks_cur in this launch
        uint32_t tx, ty, tz;
        tile_coords(t, G.ntx, G.nty, tx, ty, tz);
        const uint32_t x0 = tx * kLabelTile.tx, y0 = ty * kLabelTile.ty, z0 = tz * kLabelTile.tz;
        // the window: the tile's words and the halo's, VK_GEO_INF outside the volume.  A halo word may be the value of before its owner's
        // store in this launch.
        for (uint32_t k = 0; k < kGeoWinPerThread; k++) {
            const uint32_t c = threadIdx.x + k * kLabelThreads;
            if (c >= kGeoWindow) break;
            uint32_t wx, wy, wz;
            geo_window_coords(c, wx, wy, wz);
            const int64_t x = (int64_t)x0 + wx - 1, y = (int64_t)y0 + wy - 1, z = (int64_t)z0 + wz - 1;
            uint32_t g = kGeoInf;
            if (x >= 0 && y >= 0 && z >= 0 && x < (int64_t)G.nx && y < (int64_t)G.ny && z < (int64_t)G.nz)
                g = __hip_atomic_load(state + voxel_index((uint32_t)x, (uint32_t)y, (uint32_t)z, G.nx, G.ny), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            win[c] = g;
        }
        uint32_t in_s = 0u, lowered = 0u;  // a bit per voxel of this thread
        for (uint32_t k = 0; k < kLabelPerThread; k++) {
            uint32_t lx, ly, lz;
            label_local_coords(threadIdx.x + k * kLabelThreads, lx, ly, lz);
            const uint32_t x = x0 + lx, y = y0 + ly, z = z0 + lz;
            if (x < G.nx && y < G.ny && z < G.nz && fg[voxel_index(x, y, z, G.nx, G.ny)]) in_s |= 1u << k;
        }
        if (threadIdx.x == 0) { s_dirs = 0u; s_written = 0ull; }
        uint32_t passes = 0u;
        for (;;) {  // ends: a pass that lowers nothing (at most 4097 passes)
            if (threadIdx.x == 0) s_flag = 0u;
            __syncthreads();  // the window's load, or the pass before; the flag's reset
            bool any = false;
#pragma unroll 1
            for (uint32_t k = 0; k < kLabelPerThread; k++) {
                if (!((in_s >> k) & 1u)) continue;
                uint32_t lx, ly, lz;
                label_local_coords(threadIdx.x + k * kLabelThreads, lx, ly, lz);
                const uint32_t c = geo_window_index(lx + 1u, ly + 1u, lz + 1u);
                const uint32_t cur = GeoLds::load(win, c);
                const uint32_t best = geo_relax_voxel<GeoLds, CONN_SUM>((const uint32_t *)win, lx + 1u, ly + 1u, lz + 1u, kGeoWinX, kGeoWinY, kGeoWinZ, G.W, cur);
                if (best < cur) { GeoLds::store(win, c, best); lowered |= 1u << k; any = true; }
            }
            if (any) s_flag = 1u;
            passes++;
            __syncthreads();
            const bool again = s_flag != 0u;
            __syncthreads();  // read by everyone before the reset
            if (!again) break;
        }
        // the lowered voxels: plain 32-bit stores of words nobody else writes; the tiles they face
        uint32_t dirs = 0u, stored = 0u;
        for (uint32_t k = 0; k < kLabelPerThread; k++) {
            if (!((lowered >> k) & 1u)) continue;
            uint32_t lx, ly, lz;
            label_local_coords(threadIdx.x + k * kLabelThreads, lx, ly, lz);
            state[voxel_index(x0 + lx, y0 + ly, z0 + lz, G.nx, G.ny)] = win[geo_window_index(lx + 1u, ly + 1u, lz + 1u)];
            dirs |= geo_wake_mask(lx, ly, lz, CONN_SUM);
            stored++;
        }
        dirs = wave_reduce(dirs, WaveOr());
        if ((threadIdx.x & (warpSize - 1)) == 0 && dirs) atomicOr(&s_dirs, dirs);
        block_add(&s_written, stored);
        __syncthreads();
        const uint32_t woken = geo_mark_tiles(G, tx, ty, tz, s_dirs, marks_next, G.round + 1u);
        if (threadIdx.x == 0) {  // integers: the order of the adds does not show
            if (woken) atomicAdd(counts, (unsigned long long)woken);
            atomicAdd(counts + 1, 1ull);
            atomicAdd(counts + 2, (unsigned long long)passes);
            if (s_written) atomicAdd(counts + 3, s_written);
        }
        __syncthreads();  // the next tile's window and resets
    }
}

// partial[6 b + ...]: n_reached, n_saturated, sum_g, max_g, target_min, n_target_reached over workgroup b's voxels
__global__ __launch_bounds__(kGeoVoxelThreads) void geo_stats_kernel(const GeoDesc G, const uint32_t *__restrict__ state, const uint8_t *__restrict__ fg, unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n[4];
    __shared__ uint32_t s_max, s_min;
    if (threadIdx.x < 4u) s_n[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) { s_max = 0u; s_min = kGeoInf; }
    __syncthreads();
    unsigned long long n_reached = 0ull, n_sat = 0ull, sum = 0ull, n_target = 0ull;
    uint32_t top = 0u, low = kGeoInf;
    for (uint64_t i = (uint64_t)blockIdx.x * kGeoVoxelThreads + threadIdx.x; i < G.n; i += (uint64_t)gridDim.x * kGeoVoxelThreads) {
        const uint32_t g = state[i];
        if (!fg[i] || g == kGeoInf) continue;
        n_reached++; n_sat += g == kGeoFar; sum += g;
        top = g > top ? g : top;
        uint32_t x, y, z;
        label_coords((uint32_t)i, G.nx, G.ny, x, y, z);
        if (geo_on_faces(x, y, z, G.box, G.target_faces)) { n_target++; low = g < low ? g : low; }
    }
    block_add(&s_n[0], n_reached); block_add(&s_n[1], n_sat); block_add(&s_n[2], sum); block_add(&s_n[3], n_target);
    if (top) atomicMax(&s_max, top);
    if (low != kGeoInf) atomicMin(&s_min, low);
    publish_partials<kGeoStatsWords, 3u>(partial, s_n);
    if (threadIdx.x == 3u) partial[(size_t)kGeoStatsWords * blockIdx.x + 3u] = s_max;
    if (threadIdx.x == 4u) partial[(size_t)kGeoStatsWords * blockIdx.x + 4u] = s_min;
    if (threadIdx.x == 5u) partial[(size_t)kGeoStatsWords * blockIdx.x + 5u] = s_n[3];
}

template <int CLASS>
__global__ __launch_bounds__(kGeoVoxelThreads) void geo_dense_kernel(const GeoDesc G, const uint32_t *__restrict__ state, const uint8_t *__restrict__ fg, void *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kGeoVoxelThreads + threadIdx.x; i < G.n; i += (uint64_t)gridDim.x * kGeoVoxelThreads) {
        const uint32_t g = state[i];
        uint32_t bits = fg[i] ? G.fill_unreached_bits : G.fill_out_bits;
        if (fg[i] && g != kGeoInf) {
            const float f = (float)g;  // one rounding to nearest even
            const float w = f * G.gain;
            bits = store_gained_bits<CLASS>(w);
        }
        store_texel_bits<CLASS>(out, i, bits);
    }
}

extern "C" {

int vk_geodesic_distance(vk_ctx *ctx, const vk_geodesic_request *req, const vk_voxel_box *box, uint32_t *g_out, void *dense_out, vk_geodesic_result *result) {
    static const char *const entry = "vk_geodesic_distance";
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = geo_validate(req, g_out != nullptr, dense_out != nullptr, result != nullptr)) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + why);
    const bool install = (req->flags & VK_GEO_INSTALL) != 0u;
    if (int rc = pass_install_refused(ctx, entry, "VK_GEO_INSTALL", install)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, entry, "geodesic")) return rc;
    if (!geo_seeds_inside(req, ctx->nx, ctx->ny, ctx->nz)) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": a seed lies outside the volume");
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, entry, "VK_GEO_CLIP_BOX", box, (req->flags & VK_GEO_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, entry, "geodesic")) return rc;
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    if (n > kDistMaxVoxels) return fail(ctx, VK_ERR_UNSUPPORTED, "geodesic: a volume of more than 2^32 - 2 voxels (voxel indices are 32-bit)");

    const FilterGrid F = filter_grid(ctx->nx, ctx->ny, ctx->nz, kLabelTile, ctx->geo_max_blocks);
    GeoDesc G{};
    G.nx = ctx->nx; G.ny = ctx->ny; G.nz = ctx->nz;
    G.conn_sum = label_conn_sum(req->connectivity);
    G.ntx = F.ntx; G.nty = F.nty; G.ntz = F.ntz;
    G.tiles = (uint32_t)F.tiles;  // <= n / 4096 + ...: 32 bits hold it
    G.box = B;
    G.lo_k = label_scale_bound(req->lo, ctx->format); G.hi_k = label_scale_bound(req->hi, ctx->format);
    G.source_faces = req->source_faces; G.target_faces = req->target_faces; G.n_seeds = req->n_seeds;
    for (uint32_t s = 0; s < req->n_seeds; s++) G.seeds[s] = (uint32_t)voxel_index(req->seeds[s][0], req->seeds[s][1], req->seeds[s][2], ctx->nx, ctx->ny);
    G.fill_out_bits = label_fill_bits(req->fill_out, ctx->format);
    G.fill_unreached_bits = label_fill_bits(req->fill_unreached, ctx->format);
    G.n = n;
    G.W = geo_weights(req->spacing, G.conn_sum);
    const uint32_t tile_blocks = F.blocks;
    const uint32_t seed_blocks = std::min<uint32_t>(tile_blocks, kPassMaxPartials);  // a set of partial results per workgroup
    const uint32_t voxel_blocks = std::min<uint32_t>(label_blocks((n + kGeoVoxelThreads - 1u) / kGeoVoxelThreads, ctx->geo_max_blocks), kPassMaxPartials);

    const int kind = ctx->vol_kind;
    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, entry};
    hipError_t &e = call.e;
    // (debug, vk_debug_set_param("geo_timing", k): phase k alone between the context's timer events, read with vk_timer_elapsed_ms --
    //  1 seed, 2 relax (every round, with the host's looks at the counts), 3 stats, 4 dense; 9: nothing is timed, and a call that
    //  succeeds leaves "geodesic: rounds R launches L visits V passes P stored S" as the context's last message)
    const uint32_t timing = ctx->geo_timing;

    const size_t dense_bytes = pass_dense_bytes(ctx->format, n);
    DeviceTemp d_state, d_fg, d_marks, d_counts, d_seed, d_partial, d_out;
    if (int rc = call.alloc(d_state, (size_t)n * 4u, "the state array")) return rc;
    if (int rc = call.alloc(d_fg, (size_t)n, "the foreground bytes")) return rc;
    if (int rc = call.alloc(d_marks, (size_t)G.tiles * 8u, "the tile marks")) return rc;
    if (int rc = call.alloc(d_counts, (size_t)kGeoBatch * kGeoRoundWords * 8u, "the rounds' counts")) return rc;
    PassPartials seeds(seed_blocks, kGeoSeedWords), sums(voxel_blocks, kGeoStatsWords);
    if (int rc = call.alloc(d_seed, seeds.bytes(), "the partial totals")) return rc;
    if (int rc = call.alloc(d_partial, sums.bytes(), "the partial totals")) return rc;
    if (dense_out || install)
        if (int rc = call.alloc(d_out, dense_bytes, "the output buffer")) return rc;
    uint32_t *state = (uint32_t *)d_state.p, *marks[2] = {(uint32_t *)d_marks.p, (uint32_t *)d_marks.p + G.tiles};
    uint8_t *fg = (uint8_t *)d_fg.p;
    unsigned long long *counts = (unsigned long long *)d_counts.p;

    call.phase(timing == 1u, [&] {
        e = hipMemsetAsync(d_marks.p, 0, (size_t)G.tiles * 8u, ctx->stream);  // round numbers start at 1
        if (e != hipSuccess) return;
        with_scalar_kind(kind, [&](auto VOL) {
            hipLaunchKernelGGL(geo_seed_kernel<VOL()>, dim3(seed_blocks), dim3(kLabelThreads), 0, ctx->stream, V, G, state, fg, marks[1], (unsigned long long *)d_seed.p);
        });
    });

    // The rounds (PassCall::iterate).  Every batch but the last wakes a tile in each of its rounds; a round that wakes none leaves no
    // active tile for the rounds behind it in the batch, which exit at once: the state holds the fixed point when the batch is over.
    unsigned long long rounds = 0ull, launches = 0ull, visits = 0ull, passes = 0ull, stored = 0ull;
    call.iterate<kGeoBatch, kGeoRoundWords>(timing == 2u, counts, 0u,
        [&](uint32_t r, unsigned long long *slot) {
            G.round = r + 1u;
            const uint32_t *cur = marks[G.round & 1u];
            uint32_t *next = marks[(G.round + 1u) & 1u];
            if (G.conn_sum == 1u) hipLaunchKernelGGL(geo_relax_kernel<1u>, dim3(tile_blocks), dim3(kLabelThreads), 0, ctx->stream, G, state, (const uint8_t *)fg, cur, next, slot);
            else if (G.conn_sum == 2u) hipLaunchKernelGGL(geo_relax_kernel<2u>, dim3(tile_blocks), dim3(kLabelThreads), 0, ctx->stream, G, state, (const uint8_t *)fg, cur, next, slot);
            else hipLaunchKernelGGL(geo_relax_kernel<3u>, dim3(tile_blocks), dim3(kLabelThreads), 0, ctx->stream, G, state, (const uint8_t *)fg, cur, next, slot);
            launches++;
        },
        [&](const unsigned long long *c) {
            visits += c[1]; passes += c[2]; stored += c[3];
            if (c[1]) rounds++;
            return c[0] == 0ull;
        });

    call.phase(timing == 3u, [&] {
        hipLaunchKernelGGL(geo_stats_kernel, dim3(voxel_blocks), dim3(kGeoVoxelThreads), 0, ctx->stream, G, (const uint32_t *)state, (const uint8_t *)fg, (unsigned long long *)d_partial.p);
    });
    seeds.download(call, d_seed.p);
    sums.download(call, d_partial.p);
    call.download(g_out, state, (size_t)n * 4u);
    if (int rc = call.finish()) return rc;

    vk_geodesic_result r{};
    r.n_foreground = seeds.sum(0u); r.n_sources = seeds.sum(1u);
    r.n_reached = sums.sum(0u); r.n_saturated = sums.sum(1u); r.sum_g = sums.sum(2u); r.n_target_reached = sums.sum(5u);
    r.max_g = (uint32_t)sums.max(3u);
    r.target_min = (uint32_t)std::min<unsigned long long>(kGeoInf, sums.min(4u));
    r.gain = req->gain != 0.0f ? req->gain : geo_auto_gain(r.max_g);
    G.gain = r.gain;
    if (dense_out || install) {
        call.phase(timing == 4u, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(geo_dense_kernel<texel_class(VOL())>, dim3(voxel_blocks), dim3(kGeoVoxelThreads), 0, ctx->stream, G, (const uint32_t *)state, (const uint8_t *)fg, d_out.p);
            });
        });
        call.download(dense_out, d_out.p, dense_bytes);
        if (int rc = call.finish()) return rc;
    }
    if (result) *result = r;
    const int rc = install ? call.install(d_out, G.nx, G.ny, G.nz, ctx->format, ctx->layout) : VK_OK;
    if (rc == VK_OK && timing == 9u)
        ctx->err = "geodesic: rounds " + std::to_string(rounds) + " launches " + std::to_string(launches) + " visits " + std::to_string(visits) + " passes " + std::to_string(passes) +
                   " stored " + std::to_string(stored);
    return rc;
}

}  // extern "C"
