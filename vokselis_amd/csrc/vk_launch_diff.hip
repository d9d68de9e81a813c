// vk_launch_diff.hip -- steady-state diffusion through a value range (vk_steady_diffusion): the Laplace equation
// on the set S, no-flux walls, concentration 1 on the inlet face and 0 on the outlet face, by red-black successive over-relaxation in
// float32, every value defined bit for bit.  The request's validation, the weights, q(), a voxel's update and the stopping predicate are
// vk_diff.hpp's, shared with the host fuzz.
//
//   seed    one kernel per volume kind, a workgroup per tile: the state word of every voxel (0.5f on S, VK_DIFF_OFF elsewhere) -- no
//           later kernel touches the volume --, |S|, |inlet| and |outlet| as partial sums per workgroup, and a word per tile that says
//           whether the tile holds a voxel of S.
//   sweep   the hot path, one launch per colour, in place, a workgroup per tile: a tile without a voxel of S is left at once.  A
//           thread updates 8 voxels of the launch's colour.  Two builds of the same arithmetic: diff_sweep_kernel<false> loads the six
//           neighbours from global memory (consecutive lanes hold every second x of a row, the rows above and below and the planes
//           before and behind come from L2), diff_sweep_kernel<true> stages the tile and a one-voxel halo in LDS first, as
//           geo_relax_kernel does.  The last sweep of a block folds delta into the round's counter slot.
//   check   a kernel over the two face planes sums Fin_q and Fout_q into the round's slot; a one-thread kernel behind it evaluates the
//           predicate and sets the device's "done" word.
//   stats   sum_c_q as one partial per workgroup.
//   dense   one kernel per texel class: c * gain through the fill rule, or the fill.
// A launch updates one colour and reads the other: no workgroup reads a word that any workgroup of the same launch writes.  There is no
// stale-read argument to make and no double buffer.  No workgroup waits for another.
// The rounds.  A round of PassCall::iterate is one block: 2 * check_every sweep launches, the check and the decision.  iterate enqueues
// kDiffBatch rounds blind.  Every sweep, check and decision kernel begins by reading the "done" word, which only the decision kernel of
// an earlier launch on the same stream writes: behind the converged block every launch of the batch exits at once and changes nothing,
// so the number of sweeps that ran is the rule's.
// Every loop has a bound: the grid-stride loops their item count (tiles, voxels, face voxels); the per-thread loops 8 (a tile's voxels of
// one colour over 256 threads), 24 (the window's cells over 256 threads) or 16; the host's rounds max_sweeps / check_every.
// Every barrier stands where control flow is block-uniform: the "done" word and a tile's word are read by every thread from an array
// no workgroup of the launch writes, the tile number is blockIdx.x plus a multiple of gridDim.x.  Plain C++; no inline assembly.
// diff_sweep_kernel's registers, LDS and occupancy, from hipcc -S for gfx950: the kernel's comment and profiles/diff_pass_isa.txt.
#include "vk_diff.hpp"
#include "vk_launch.hpp"
#include "vk_pass_blocks.hpp"
#include "vk_texel.hpp"

using namespace vk;

constexpr uint32_t kDiffVoxelThreads = 256, kDiffSeedWords = 3, kDiffStatsWords = 1;
constexpr uint32_t kDiffPerColour = kLabelTileVoxels / 2u / kLabelThreads;  // 8
constexpr uint32_t kDiffMaxCheckBlocks = 1024;
static_assert(kLabelTile.tx % 2u == 0u, "a tile's origin has an even x: the colour of a voxel follows from its local x");
static_assert(kLabelThreads == kLabelTile.tx / 2u * kLabelTile.ty && kDiffPerColour == kLabelTile.tz, "a thread takes one half-row position of one row in each of the tile's planes");

struct DiffDesc {
    uint32_t nx, ny, nz, axis;
    uint32_t ntx, nty, ntz, tiles;
    vk_voxel_box box;
    float lo_k, hi_k;
    DiffWeights W;
    float omega, gain;
    uint32_t inlet, outlet;  // the coordinate along the axis of the two faces
    uint32_t colour, fold;   // of a sweep launch: its parity; whether it folds delta
    uint32_t fill_out_bits, pad;
    float delta_tol, flux_tol;
    uint64_t n;
};
static_assert(sizeof(DiffDesc) % 8 == 0 && pass_kernargs_fit<DiffDesc>, "diffusion kernels: VolumeDesc + DiffDesc");

struct DiffWords {  // a state word, from global memory or from the window in LDS
    static __device__ __forceinline__ uint32_t load(const uint32_t *p, uint32_t i) { return p[i]; }
};

__device__ __forceinline__ uint32_t diff_along(const DiffDesc &D, uint32_t x, uint32_t y, uint32_t z) { return D.axis == 0u ? x : (D.axis == 1u ? y : z); }

// state: the whole volume.  tile_has[t]: 1 iff tile t holds a voxel of S.  partial[3 b + ...]: |S|, |inlet|, |outlet| over workgroup b's tiles.
template <int VOL>
__global__ __launch_bounds__(kLabelThreads) void diff_seed_kernel(const VolumeDesc V, const DiffDesc D, uint32_t *__restrict__ state, uint32_t *__restrict__ tile_has,
                                                                  unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n[kDiffSeedWords];
    __shared__ uint32_t s_any;
    if (threadIdx.x < kDiffSeedWords) s_n[threadIdx.x] = 0ull;
    uint32_t n_fg = 0u, n_in = 0u, n_out = 0u;
    for (uint32_t t = blockIdx.x; t < D.tiles; t += gridDim.x) {  // block-uniform
        if (threadIdx.x == 0) s_any = 0u;
        __syncthreads();
        uint32_t tx, ty, tz;
        tile_coords(t, D.ntx, D.nty, tx, ty, tz);
        const uint32_t x0 = tx * kLabelTile.tx, y0 = ty * kLabelTile.ty, z0 = tz * kLabelTile.tz;
        bool any = false;
        for (uint32_t k = 0; k < kLabelPerThread; k++) {
            uint32_t lx, ly, lz;
            label_local_coords(threadIdx.x + k * kLabelThreads, lx, ly, lz);
            const uint32_t x = x0 + lx, y = y0 + ly, z = z0 + lz;
            if (x >= D.nx || y >= D.ny || z >= D.nz) continue;
            const bool in_s = label_in_box(x, y, z, D.box) && label_foreground(texel_f32<VOL>(voxel_texel_bits<VOL>(V, x, y, z)), D.lo_k, D.hi_k);
            state[voxel_index(x, y, z, D.nx, D.ny)] = in_s ? diff_bits(0.5f) : kDiffOff;
            const uint32_t a = diff_along(D, x, y, z);
            n_fg += in_s; n_in += in_s && a == D.inlet; n_out += in_s && a == D.outlet;
            any = any || in_s;
        }
        if (any) s_any = 1u;  // every writer stores the same value
        __syncthreads();
        if (threadIdx.x == 0) tile_has[t] = s_any;
        __syncthreads();  // the next tile's reset
    }
    block_add(&s_n[0], n_fg); block_add(&s_n[1], n_in); block_add(&s_n[2], n_out);
    publish_partials<kDiffSeedWords>(partial, s_n);
}

// One colour of one sweep (D.colour), in place.  slot: the round's counters; with D.fold the launch folds the largest |c' - c| of its
// voxels into slot[kDiffSlotDelta] (non-negative floats order like their bits: the maximum depends on no order).
// Thread t of a tile takes, for k = 0 .. 7, the voxel of half-row position t % 16 in row t / 16 of plane k: x = x0 + 2 (t % 16) + p with
// p the parity that gives the voxel the launch's colour.  A wave covers four rows of 32 voxels: 128 bytes a row, every second word its
// own, the words between them its x neighbours.
// A thread first loads its 8 own words and their 48 neighbour words -- no load behind a branch, all in flight together -- and then does
// the arithmetic.  LDS = false: the words come from global memory; the x neighbours share the centre's lines, y and z neighbours are
// other waves' centres of the launch before (L2, or the CU's cache within a tile).  LDS = true: the window of (32 + 2) x (16 + 2) x (8 + 2)
// words goes through LDS first.
// hipcc -S, gfx950 (profiles/diff_pass_isa.txt): <false> 72 VGPRs, 106 SGPRs, no LDS: 7 waves per SIMD.  <true> 231 VGPRs, 82 SGPRs,
// 24480 bytes of LDS: 2 waves per SIMD by registers.  Neither spills to scratch.  Each of a thread's 8 quotients is the v_div_scale /
// v_div_fmas / v_div_fixup sequence, not a bare reciprocal.  Measured: <false> is the faster, and the default.
template <bool LDS>
__global__ __launch_bounds__(kLabelThreads) void diff_sweep_kernel(const DiffDesc D, uint32_t *state, const uint32_t *__restrict__ tile_has, const uint32_t *__restrict__ done,
                                                                   unsigned long long *__restrict__ slot) {
    __shared__ uint32_t win[LDS ? kGeoWindow : 1u];
    if (*done) return;  // block-uniform: written by an earlier launch only
    uint32_t top = 0u;
    for (uint32_t t = blockIdx.x; t < D.tiles; t += gridDim.x) {  // block-uniform
        if (!tile_has[t]) continue;                               // block-uniform: nobody writes tile_has in this launch
        uint32_t tx, ty, tz;
        tile_coords(t, D.ntx, D.nty, tx, ty, tz);
        const uint32_t x0 = tx * kLabelTile.tx, y0 = ty * kLabelTile.ty, z0 = tz * kLabelTile.tz;
        if constexpr (LDS) {
            // the window: the tile's words and the halo's, VK_DIFF_OFF outside the volume.  Words of the launch's own colour in the halo
            // may be mid-update by their owner; no voxel of this colour reads them.
            for (uint32_t k = 0; k < kGeoWinPerThread; k++) {
                const uint32_t c = threadIdx.x + k * kLabelThreads;
                if (c >= kGeoWindow) break;
                uint32_t wx, wy, wz;
                geo_window_coords(c, wx, wy, wz);
                const int64_t x = (int64_t)x0 + wx - 1, y = (int64_t)y0 + wy - 1, z = (int64_t)z0 + wz - 1;
                uint32_t g = kDiffOff;
                if (x >= 0 && y >= 0 && z >= 0 && x < (int64_t)D.nx && y < (int64_t)D.ny && z < (int64_t)D.nz)
                    g = state[voxel_index((uint32_t)x, (uint32_t)y, (uint32_t)z, D.nx, D.ny)];
                win[c] = g;
            }
            __syncthreads();
        }
        float c_new[kDiffPerColour];
        uint32_t write = 0u;  // a bit per voxel of this thread
        const uint32_t hx = threadIdx.x % (kLabelTile.tx / 2u), ly = threadIdx.x / (kLabelTile.tx / 2u), y = y0 + ly;
        // the words first -- a thread's own 8 and their 48 neighbours, no load behind a branch (a voxel outside the volume loads word 0
        // and drops it), so that they are all in flight together --, then the arithmetic
        uint32_t own[kDiffPerColour], nb[kDiffPerColour][6];
#pragma unroll
        for (uint32_t k = 0; k < kDiffPerColour; k++) {
            const uint32_t z = z0 + k, lx = 2u * hx + ((y + z + D.colour) & 1u), x = x0 + lx;
            const bool inside = x < D.nx && y < D.ny && z < D.nz;
            if constexpr (LDS) {
                own[k] = inside ? win[geo_window_index(lx + 1u, ly + 1u, k + 1u)] : kDiffOff;
                diff_load_neighbours<DiffWords>((const uint32_t *)win, lx + 1u, ly + 1u, k + 1u, kGeoWinX, kGeoWinY, kGeoWinZ, nb[k]);
            } else {
                const uint32_t cx = inside ? x : 0u, cy = inside ? y : 0u, cz = inside ? z : 0u;
                const uint32_t w = state[voxel_index(cx, cy, cz, D.nx, D.ny)];
                own[k] = inside ? w : kDiffOff;
                diff_load_neighbours<DiffWords>((const uint32_t *)state, cx, cy, cz, D.nx, D.ny, D.nz, nb[k]);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kDiffPerColour; k++) {
            c_new[k] = 0.0f;
            if (own[k] == kDiffOff) continue;
            const uint32_t z = z0 + k, x = x0 + 2u * hx + ((y + z + D.colour) & 1u);
            const float c = diff_float(own[k]);
            const uint32_t a = diff_along(D, x, y, z);
            if (!diff_update_from(nb[k], D.W, a == D.inlet, a == D.outlet, D.omega, c, c_new[k])) continue;
            write |= 1u << k;
            const float moved = c_new[k] - c;
            const uint32_t bits = diff_bits(fabsf(moved));
            top = bits > top ? bits : top;
        }
#pragma unroll
        for (uint32_t k = 0; k < kDiffPerColour; k++) {
            if (!((write >> k) & 1u)) continue;
            const uint32_t z = z0 + k, x = x0 + 2u * hx + ((y + z + D.colour) & 1u);
            state[voxel_index(x, y, z, D.nx, D.ny)] = diff_bits(c_new[k]);
        }
        if constexpr (LDS) __syncthreads();  // the next tile's window
    }
    if (D.fold) {  // block-uniform
        top = wave_reduce(top, WaveMax());
        if ((threadIdx.x & (warpSize - 1)) == 0 && top) atomicMax(slot + kDiffSlotDelta, (unsigned long long)top);
    }
}

// The two face planes of B: item j < cross is voxel j of the inlet plane, item cross + j voxel j of the outlet plane, the plane's two
// axes in the order (a + 1) % 3, (a + 2) % 3.  Sums Fin_q and Fout_q into the round's slot, as two's-complement integers.
__global__ __launch_bounds__(kDiffVoxelThreads) void diff_check_kernel(const DiffDesc D, const uint32_t *__restrict__ state, const uint32_t *__restrict__ done,
                                                                        unsigned long long *__restrict__ slot) {
    __shared__ unsigned long long s_n[2];
    if (*done) return;  // block-uniform
    if (threadIdx.x < 2u) s_n[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t lo3[3] = {D.box.x0, D.box.y0, D.box.z0}, hi3[3] = {D.box.x1, D.box.y1, D.box.z1};
    const uint32_t b = (D.axis + 1u) % 3u, c = (D.axis + 2u) % 3u;
    const uint64_t nb = hi3[b] - lo3[b], cross = hi3[D.axis] > lo3[D.axis] ? nb * (hi3[c] - lo3[c]) : 0u;  // an empty box has no face
    unsigned long long fin = 0ull, fout = 0ull;
    for (uint64_t j = (uint64_t)blockIdx.x * kDiffVoxelThreads + threadIdx.x; j < 2u * cross; j += (uint64_t)gridDim.x * kDiffVoxelThreads) {
        const bool out = j >= cross;
        const uint64_t jj = out ? j - cross : j;
        uint32_t p[3];
        p[D.axis] = out ? D.outlet : D.inlet;
        p[b] = lo3[b] + (uint32_t)(jj % nb);
        p[c] = lo3[c] + (uint32_t)(jj / nb);
        const uint32_t w = state[voxel_index(p[0], p[1], p[2], D.nx, D.ny)];
        if (w == kDiffOff) continue;
        const float v = diff_float(w);
        if (out) fout += (unsigned long long)diff_flux_out_q(v); else fin += (unsigned long long)diff_flux_in_q(v);
    }
    block_add(&s_n[0], fin); block_add(&s_n[1], fout);
    __syncthreads();
    if (threadIdx.x == 0 && s_n[0]) atomicAdd(slot + kDiffSlotFin, s_n[0]);
    if (threadIdx.x == 1 && s_n[1]) atomicAdd(slot + kDiffSlotFout, s_n[1]);
}

// one thread: the predicate on the round's slot; the "done" word for every launch behind this one
__global__ void diff_decide_kernel(const DiffDesc D, uint32_t *__restrict__ done, unsigned long long *__restrict__ slot) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || *done) return;
    slot[kDiffSlotRan] = 1ull;
    const bool conv = diff_converged(diff_float((uint32_t)slot[kDiffSlotDelta]), (int64_t)slot[kDiffSlotFin], (int64_t)slot[kDiffSlotFout], D.delta_tol, D.flux_tol);
    if (conv) { slot[kDiffSlotConverged] = 1ull; *done = 1u; }
}

// partial[b]: the sum of q(c) over workgroup b's voxels of S
__global__ __launch_bounds__(kDiffVoxelThreads) void diff_stats_kernel(const DiffDesc D, const uint32_t *__restrict__ state, unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n[kDiffStatsWords];
    if (threadIdx.x < kDiffStatsWords) s_n[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long sum = 0ull;
    for (uint64_t i = (uint64_t)blockIdx.x * kDiffVoxelThreads + threadIdx.x; i < D.n; i += (uint64_t)gridDim.x * kDiffVoxelThreads) {
        const uint32_t w = state[i];
        if (w != kDiffOff) sum += (unsigned long long)diff_q(diff_float(w));
    }
    block_add(&s_n[0], sum);
    publish_partials<kDiffStatsWords>(partial, s_n);
}

template <int CLASS>
__global__ __launch_bounds__(kDiffVoxelThreads) void diff_dense_kernel(const DiffDesc D, const uint32_t *__restrict__ state, void *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kDiffVoxelThreads + threadIdx.x; i < D.n; i += (uint64_t)gridDim.x * kDiffVoxelThreads) {
        const uint32_t w = state[i];
        uint32_t bits = D.fill_out_bits;
        if (w != kDiffOff) {
            const float v = diff_float(w) * D.gain;
            bits = store_gained_bits<CLASS>(v);
        }
        store_texel_bits<CLASS>(out, i, bits);
    }
}

extern "C" {

int vk_steady_diffusion(vk_ctx *ctx, const vk_diffusion_request *req, const vk_voxel_box *box, float *c_out, void *dense_out, vk_diffusion_result *result) {
    static const char *const entry = "vk_steady_diffusion";
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = diff_validate(req, c_out != nullptr, dense_out != nullptr, result != nullptr)) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + why);
    const bool install = (req->flags & VK_DIFF_INSTALL) != 0u;
    if (int rc = pass_install_refused(ctx, entry, "VK_DIFF_INSTALL", install)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, entry, "diffusion")) return rc;
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, entry, "VK_DIFF_CLIP_BOX", box, (req->flags & VK_DIFF_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, entry, "diffusion")) return rc;
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    if (n > kDistMaxVoxels) return fail(ctx, VK_ERR_UNSUPPORTED, "diffusion: a volume of more than 2^32 - 2 voxels (voxel indices are 32-bit)");

    const FilterGrid F = filter_grid(ctx->nx, ctx->ny, ctx->nz, kLabelTile, ctx->diff_max_blocks);
    const uint32_t lo3[3] = {B.x0, B.y0, B.z0}, hi3[3] = {B.x1, B.y1, B.z1};
    const uint32_t extent[3] = {B.x1 - B.x0, B.y1 - B.y0, B.z1 - B.z0};
    const uint32_t a = req->axis, n_a = extent[a];
    DiffDesc D{};
    D.nx = ctx->nx; D.ny = ctx->ny; D.nz = ctx->nz; D.axis = a;
    D.ntx = F.ntx; D.nty = F.nty; D.ntz = F.ntz;
    D.tiles = (uint32_t)F.tiles;
    D.box = B;
    D.lo_k = label_scale_bound(req->lo, ctx->format); D.hi_k = label_scale_bound(req->hi, ctx->format);
    D.W = diff_weights(req->spacing, a);
    D.omega = diff_omega(req, n_a);
    D.gain = req->gain != 0.0f ? req->gain : 1.0f;
    D.inlet = lo3[a]; D.outlet = hi3[a] - 1u;  // of an empty box: never compared with a voxel of S
    D.fill_out_bits = label_fill_bits(req->fill_out, ctx->format);
    D.delta_tol = req->delta_tol; D.flux_tol = req->flux_tol;
    D.n = n;
    const uint64_t n_box = (uint64_t)extent[0] * extent[1] * extent[2];
    const uint64_t face_items = n_a ? 2ull * extent[(a + 1u) % 3u] * extent[(a + 2u) % 3u] : 0ull;
    const uint32_t tile_blocks = F.blocks;
    const uint32_t seed_blocks = std::min<uint32_t>(tile_blocks, kPassMaxPartials);
    const uint32_t voxel_blocks = std::min<uint32_t>(label_blocks((n + kDiffVoxelThreads - 1u) / kDiffVoxelThreads, ctx->diff_max_blocks), kPassMaxPartials);
    const uint32_t check_blocks = std::min<uint32_t>(label_blocks((face_items + kDiffVoxelThreads - 1u) / kDiffVoxelThreads, ctx->diff_max_blocks), kDiffMaxCheckBlocks);
    const uint32_t check_every = req->check_every, budget = req->max_sweeps / check_every;

    const int kind = ctx->vol_kind;
    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, entry};
    hipError_t &e = call.e;
    // (debug, vk_debug_set_param("diff_timing", k): phase k alone between the context's timer events, read with vk_timer_elapsed_ms --
    //  1 seed, 2 sweeps (every block, with the checks and the host's looks at the counts), 3 stats, 4 dense; 9: nothing is timed, and a
    //  call that succeeds leaves "diffusion: blocks B launches L sweeps S" as the context's last message.  "diff_lds", 1: the sweeps
    //  stage their tiles in LDS -- the same bits, for measurements)
    const uint32_t timing = ctx->diff_timing;
    const bool lds = ctx->diff_lds != 0u;

    const size_t dense_bytes = pass_dense_bytes(ctx->format, n);
    DeviceTemp d_state, d_tiles, d_counts, d_done, d_seed, d_partial, d_out;
    if (int rc = call.alloc(d_state, (size_t)n * 4u, "the state array")) return rc;
    if (int rc = call.alloc(d_tiles, (size_t)D.tiles * 4u, "the tile words")) return rc;
    if (int rc = call.alloc(d_counts, (size_t)kDiffBatch * kDiffRoundWords * 8u, "the rounds' counts")) return rc;
    if (int rc = call.alloc(d_done, 4u, "the done word")) return rc;
    PassPartials seeds(seed_blocks, kDiffSeedWords), sums(voxel_blocks, kDiffStatsWords);
    if (int rc = call.alloc(d_seed, seeds.bytes(), "the partial totals")) return rc;
    if (int rc = call.alloc(d_partial, sums.bytes(), "the partial totals")) return rc;
    if (dense_out || install)
        if (int rc = call.alloc(d_out, dense_bytes, "the output buffer")) return rc;
    uint32_t *state = (uint32_t *)d_state.p, *tile_has = (uint32_t *)d_tiles.p, *done = (uint32_t *)d_done.p;
    unsigned long long *counts = (unsigned long long *)d_counts.p;

    call.phase(timing == 1u, [&] {
        e = hipMemsetAsync(d_done.p, 0, 4u, ctx->stream);
        if (e != hipSuccess) return;
        with_scalar_kind(kind, [&](auto VOL) {
            hipLaunchKernelGGL(diff_seed_kernel<VOL()>, dim3(seed_blocks), dim3(kLabelThreads), 0, ctx->stream, V, D, state, tile_has, (unsigned long long *)d_seed.p);
        });
    });

    // The blocks (PassCall::iterate): the launches of a round behind the converged one exit on the "done" word.
    unsigned long long blocks = 0ull, launches = 0ull;
    unsigned long long last_delta = 0ull, last_fin = 0ull, last_fout = 0ull;
    bool converged = false;
    call.iterate<kDiffBatch, kDiffRoundWords>(timing == 2u, counts, budget,
        [&](uint32_t, unsigned long long *slot) {
            for (uint32_t s = 0; s < check_every; s++)
                for (uint32_t colour = 0; colour < 2u; colour++)
                    call.enqueue([&] {
                        D.colour = colour; D.fold = s + 1u == check_every ? 1u : 0u;
                        if (lds) hipLaunchKernelGGL(diff_sweep_kernel<true>, dim3(tile_blocks), dim3(kLabelThreads), 0, ctx->stream, D, state, (const uint32_t *)tile_has, (const uint32_t *)done, slot);
                        else hipLaunchKernelGGL(diff_sweep_kernel<false>, dim3(tile_blocks), dim3(kLabelThreads), 0, ctx->stream, D, state, (const uint32_t *)tile_has, (const uint32_t *)done, slot);
                        launches++;
                    });
            call.enqueue([&] {
                hipLaunchKernelGGL(diff_check_kernel, dim3(check_blocks), dim3(kDiffVoxelThreads), 0, ctx->stream, D, (const uint32_t *)state, (const uint32_t *)done, slot);
                launches++;
            });
            call.enqueue([&] {
                hipLaunchKernelGGL(diff_decide_kernel, dim3(1), dim3(64), 0, ctx->stream, D, done, slot);
                launches++;
            });
        },
        [&](const unsigned long long *c) {
            if (!c[kDiffSlotRan]) return true;  // (not reached: a round that did not run stands behind a converged one)
            blocks++;
            last_delta = c[kDiffSlotDelta]; last_fin = c[kDiffSlotFin]; last_fout = c[kDiffSlotFout];
            converged = c[kDiffSlotConverged] != 0ull;
            return converged;
        });

    call.phase(timing == 3u, [&] {
        hipLaunchKernelGGL(diff_stats_kernel, dim3(voxel_blocks), dim3(kDiffVoxelThreads), 0, ctx->stream, D, (const uint32_t *)state, (unsigned long long *)d_partial.p);
    });
    seeds.download(call, d_seed.p);
    sums.download(call, d_partial.p);
    call.download(c_out, state, (size_t)n * 4u);
    if (int rc = call.finish()) return rc;

    vk_diffusion_result r{};
    r.n_foreground = seeds.sum(0u); r.n_inlet = seeds.sum(1u); r.n_outlet = seeds.sum(2u); r.n_box = n_box;
    r.Fin_q = (int64_t)last_fin; r.Fout_q = (int64_t)last_fout; r.sum_c_q = (int64_t)sums.sum(0u);
    r.sweeps = (uint32_t)(blocks * check_every); r.converged = converged ? 1u : 0u;
    r.delta = diff_float((uint32_t)last_delta); r.omega = D.omega; r.gain = D.gain;
    if (dense_out || install) {
        call.phase(timing == 4u, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(diff_dense_kernel<texel_class(VOL())>, dim3(voxel_blocks), dim3(kDiffVoxelThreads), 0, ctx->stream, D, (const uint32_t *)state, d_out.p);
            });
        });
        call.download(dense_out, d_out.p, dense_bytes);
        if (int rc = call.finish()) return rc;
    }
    if (result) *result = r;
    const int rc = install ? call.install(d_out, D.nx, D.ny, D.nz, ctx->format, ctx->layout) : VK_OK;
    if (rc == VK_OK && timing == 9u)
        ctx->err = "diffusion: blocks " + std::to_string(blocks) + " launches " + std::to_string(launches) + " sweeps " + std::to_string(blocks * check_every);
    return rc;
}

}  // extern "C"
