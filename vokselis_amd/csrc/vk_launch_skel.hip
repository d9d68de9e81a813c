// vk_launch_skel.hip -- skeleton of a value range (vk_skeletonize): the set S thinned, by deleting simple points
// subfield by subfield, to a one-voxel-wide set K with the same pieces, tunnels and cavities.  The request's validation, the mask's bit
// order, the simple-point test (a bit flood by shifts, no table), a voxel's visit, its class and the mapping of threads onto a tile's
// voxels of one subfield are vk_skel.hpp's, shared with the host fuzz.
//
//   seed    one kernel per volume kind, a workgroup per tile, the only phase before `dense` that reads the volume: the state byte of
//           every voxel (1 on S, 0 elsewhere), |S| as partial sums per workgroup, and the stamp of iteration 1 on every tile that holds
//           a voxel of S.
//   thin    the hot path, one launch per sub-pass, eight per iteration, a workgroup per tile: a tile whose stamp is not this iteration's
//           is left at once.  An active tile loads its 34 x 18 x 10 state bytes into LDS, maps its threads onto its 512 voxels of the
//           sub-pass's subfield, two per thread, gathers each voxel's 26 bits there, tests, stores the bytes that change and, if it
//           deleted anything, stamps itself and the up to 26 tiles around it for the next iteration.
//   stats   the class of every voxel (to class_out's buffer where asked for) and the totals as partial results per workgroup.
//   dense   one kernel per volume kind: the stored bits or F(fill_in) on K, F(fill_out) elsewhere.
// "Was in K_i" needs no launch of its own: a deleted voxel's byte names the parity of its iteration (vk_skel.hpp, the state byte), and
// the workgroup that owns it clears it one iteration later; every reader reads both values alike.  A voxel's byte is written by the
// workgroup that owns its tile, in the sub-pass of its subfield, and by nobody else; another workgroup of the same launch may load it
// for its halo, but a sub-pass uses only bytes of the other seven subfields, which no workgroup writes in that launch.  A launch
// boundary between sub-passes is all the ordering there is: no workgroup waits for another, no spinning, no persistent kernel.
// The active set is one word per tile and parity of the iteration, as the geodesic pass keeps it: the eight launches of iteration i run
// the tiles whose word in array i & 1 equals i and write i + 1 into array (i + 1) & 1.
// Every loop has a bound: the grid-stride loops their item count; the two floods of skel_simple27 26 and 18 trips; the host's iterations
// end because every iteration but the last deletes a voxel of a finite set.  Every barrier stands where control flow is block-uniform:
// the tile number and the tile's stamp (no workgroup of the launch writes the array it is read from).  Plain C++; no inline assembly.
// skel_thin_kernel's registers, LDS and occupancy, from hipcc -S for gfx950: the kernel's comment and profiles/skel_pass_isa.txt.
#include "vk_launch.hpp"
#include "vk_pass_blocks.hpp"
#include "vk_skel.hpp"
#include "vk_texel.hpp"

using namespace vk;

constexpr uint32_t kSkelVoxelThreads = 256, kSkelStatsWords = 5u + VK_SKEL_LINKS;
constexpr uint32_t kSkelWinBytes = (kGeoWindow + 3u) & ~3u;

struct SkelDesc {
    uint32_t nx, ny, nz, curve;
    uint32_t ntx, nty, ntz, tiles;
    vk_voxel_box box;
    float lo_k, hi_k;
    uint32_t iteration, subpass;
    uint32_t fill_in_bits, fill_out_bits, fill_in_on, pad;
    uint64_t n;
};
static_assert(sizeof(SkelDesc) % 8 == 0 && pass_kernargs_fit<SkelDesc>, "skeleton kernels: VolumeDesc + SkelDesc");

// the window in LDS: bytes, written before a barrier and only read behind it
struct SkelLds {
    static __device__ __forceinline__ uint32_t load(const uint8_t *p, uint32_t i) { return p[i]; }
};

// state: the whole volume.  marks: the array of iteration 1.  partial[b]: |S| over workgroup b's tiles.
template <int VOL>
__global__ __launch_bounds__(kLabelThreads) void skel_seed_kernel(const VolumeDesc V, const SkelDesc G, uint8_t *__restrict__ state, uint32_t *__restrict__ marks,
                                                                  unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n;
    __shared__ uint32_t s_any;
    if (threadIdx.x == 0) s_n = 0ull;
    uint32_t n_fg = 0u;
    for (uint32_t t = blockIdx.x; t < G.tiles; t += gridDim.x) {  // block-uniform
        if (threadIdx.x == 0) s_any = 0u;
        __syncthreads();
        uint32_t tx, ty, tz;
        tile_coords(t, G.ntx, G.nty, tx, ty, tz);
        const uint32_t x0 = tx * kLabelTile.tx, y0 = ty * kLabelTile.ty, z0 = tz * kLabelTile.tz;
        bool any = false;
        for (uint32_t k = 0; k < kLabelPerThread; k++) {
            uint32_t lx, ly, lz;
            label_local_coords(threadIdx.x + k * kLabelThreads, lx, ly, lz);
            const uint32_t x = x0 + lx, y = y0 + ly, z = z0 + lz;
            if (x >= G.nx || y >= G.ny || z >= G.nz) continue;
            const bool in_s = label_in_box(x, y, z, G.box) && label_foreground(texel_f32<VOL>(voxel_texel_bits<VOL>(V, x, y, z)), G.lo_k, G.hi_k);
            state[voxel_index(x, y, z, G.nx, G.ny)] = in_s ? (uint8_t)kSkelIn : (uint8_t)kSkelOff;
            n_fg += in_s;
            any = any || in_s;
        }
        if (any) s_any = 1u;  // every writer stores the same value
        __syncthreads();
        if (threadIdx.x == 0 && s_any) marks[t] = 1u;
        __syncthreads();  // the next tile's reset
    }
    block_add(&s_n, n_fg);
    publish_partials<1u>(partial, &s_n);
}

// One sub-pass (G.subpass) of one iteration (G.iteration).  marks_cur: the tiles of this iteration; marks_next: those of the next.
// counts[0 .. 2): the voxels this iteration deleted and the tile visits of its launches.
// hipcc -S, gfx950 (profiles/skel_pass_isa.txt): 49 VGPRs, 106 SGPRs, none spilled to scratch (ScratchSize 0), 6124 bytes of LDS -- the
// window and the deletion count.  The registers bound the occupancy, at 7 waves per SIMD; LDS would allow 26 workgroups on a CU.
__global__ __launch_bounds__(kLabelThreads) void skel_thin_kernel(const SkelDesc G, uint8_t *__restrict__ state, const uint32_t *__restrict__ marks_cur, uint32_t *__restrict__ marks_next,
                                                                  unsigned long long *__restrict__ counts) {
    __shared__ __attribute__((aligned(4))) uint8_t win[kSkelWinBytes];
    __shared__ uint32_t s_deleted;
    for (uint32_t t = blockIdx.x; t < G.tiles; t += gridDim.x) {  // block-uniform
        if (marks_cur[t] != G.iteration) continue;                 // block-uniform: nobody writes marks_cur in this launch
        uint32_t tx, ty, tz;
        tile_coords(t, G.ntx, G.nty, tx, ty, tz);
        const uint32_t x0 = tx * kLabelTile.tx, y0 = ty * kLabelTile.ty, z0 = tz * kLabelTile.tz;
        // the window: the tile's bytes and the halo's, 0 outside the volume.  A halo byte of this sub-pass's subfield may be the value of
        // before or after its owner's store in this launch; no voxel's visit reads a byte of its own subfield but its own.
        for (uint32_t k = 0; k < kGeoWinPerThread; k++) {
            const uint32_t c = threadIdx.x + k * kLabelThreads;
            if (c >= kGeoWindow) break;
            uint32_t wx, wy, wz;
            geo_window_coords(c, wx, wy, wz);
            const int64_t x = (int64_t)x0 + wx - 1, y = (int64_t)y0 + wy - 1, z = (int64_t)z0 + wz - 1;
            uint8_t st = (uint8_t)kSkelOff;
            if (x >= 0 && y >= 0 && z >= 0 && x < (int64_t)G.nx && y < (int64_t)G.ny && z < (int64_t)G.nz)
                st = __hip_atomic_load(state + voxel_index((uint32_t)x, (uint32_t)y, (uint32_t)z, G.nx, G.ny), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            win[c] = st;
        }
        if (threadIdx.x == 0) s_deleted = 0u;
        __syncthreads();
        uint32_t deleted = 0u;
#pragma unroll 1
        for (uint32_t k = 0; k < kSkelPerThread; k++) {
            uint32_t lx, ly, lz;
            skel_sub_coords(threadIdx.x + k * kLabelThreads, G.subpass, lx, ly, lz);
            const uint32_t before = win[geo_window_index(lx + 1u, ly + 1u, lz + 1u)];
            if (before == kSkelOff) continue;  // also every cell of the tile that lies outside the volume
            const uint32_t after = skel_visit<SkelLds>((const uint8_t *)win, lx + 1u, ly + 1u, lz + 1u, G.iteration, G.curve != 0u);
            if (after == before) continue;
            state[voxel_index(x0 + lx, y0 + ly, z0 + lz, G.nx, G.ny)] = (uint8_t)after;  // a byte nobody else writes
            deleted += after != kSkelOff;
        }
        deleted = (uint32_t)__popcll(__ballot(deleted & 1u)) + 2u * (uint32_t)__popcll(__ballot(deleted >> 1));
        if ((threadIdx.x & (warpSize - 1)) == 0 && deleted) atomicAdd(&s_deleted, deleted);
        __syncthreads();
        const uint32_t n_deleted = s_deleted;
        if (n_deleted && threadIdx.x < kLabelOffsets) {
            uint32_t nb;
            if (geo_tile_neighbour(tx, ty, tz, G.ntx, G.nty, G.ntz, threadIdx.x, nb)) marks_next[nb] = G.iteration + 1u;  // several writers, one value
        }
        if (threadIdx.x == 0) {  // integers: the order of the adds does not show
            if (n_deleted) atomicAdd(counts, (unsigned long long)n_deleted);
            atomicAdd(counts + 1, 1ull);
        }
        __syncthreads();  // the next tile's window and reset
    }
}

// partial[18 b + ...]: |K|, the four classes, the 13 links over workgroup b's voxels.  cls: NULL, or the class of every voxel.
__global__ __launch_bounds__(kSkelVoxelThreads) void skel_stats_kernel(const SkelDesc G, const uint8_t *__restrict__ state, uint8_t *__restrict__ cls, unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n[kSkelStatsWords];
    if (threadIdx.x < kSkelStatsWords) s_n[threadIdx.x] = 0ull;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kSkelVoxelThreads + threadIdx.x; i < G.n; i += (uint64_t)gridDim.x * kSkelVoxelThreads) {
        const bool in_k = skel_in(state[i]);
        uint32_t m27 = 0u;
        if (in_k) {
            uint32_t x, y, z;
            label_coords((uint32_t)i, G.nx, G.ny, x, y, z);
            for (uint32_t o = 0; o < kLabelOffsets; o++) {
                if (o == kLabelCentre) continue;
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                const int64_t hx = (int64_t)x + dx, hy = (int64_t)y + dy, hz = (int64_t)z + dz;  // no wrap: a neighbour outside the volume is background
                if (hx < 0 || hy < 0 || hz < 0 || hx >= (int64_t)G.nx || hy >= (int64_t)G.ny || hz >= (int64_t)G.nz) continue;
                if (skel_in(state[voxel_index((uint32_t)hx, (uint32_t)hy, (uint32_t)hz, G.nx, G.ny)])) m27 |= 1u << o;
            }
        }
        const uint32_t c = skel_class(in_k, (uint32_t)__popc(m27));
        if (cls) cls[i] = (uint8_t)c;
        if (!in_k) continue;  // K is thin: few threads get here
        atomicAdd(&s_n[0], 1ull);
        atomicAdd(&s_n[c], 1ull);
        for (uint32_t above = m27 >> (kLabelCentre + 1u), j = 0; above; above >>= 1, j++)
            if (above & 1u) atomicAdd(&s_n[5u + j], 1ull);
    }
    publish_partials<kSkelStatsWords>(partial, s_n);
}

template <int VOL>
__global__ __launch_bounds__(kSkelVoxelThreads) void skel_dense_kernel(const VolumeDesc V, const SkelDesc G, const uint8_t *__restrict__ state, void *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kSkelVoxelThreads + threadIdx.x; i < G.n; i += (uint64_t)gridDim.x * kSkelVoxelThreads) {
        uint32_t bits = G.fill_out_bits;
        if (skel_in(state[i])) {
            bits = G.fill_in_bits;
            if (!G.fill_in_on) {
                uint32_t x, y, z;
                label_coords((uint32_t)i, G.nx, G.ny, x, y, z);
                bits = voxel_texel_bits<VOL>(V, x, y, z);
            }
        }
        store_texel_bits<texel_class(VOL)>(out, i, bits);
    }
}

extern "C" {

int vk_skeletonize(vk_ctx *ctx, const vk_skeleton_request *req, const vk_voxel_box *box, uint8_t *class_out, void *dense_out, vk_skeleton_result *result) {
    static const char *const entry = "vk_skeletonize";
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = skel_validate(req, class_out != nullptr, dense_out != nullptr, result != nullptr)) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + why);
    const bool install = (req->flags & VK_SKEL_INSTALL) != 0u;
    if (int rc = pass_install_refused(ctx, entry, "VK_SKEL_INSTALL", install)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, entry, "skeleton")) return rc;
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, entry, "VK_SKEL_CLIP_BOX", box, (req->flags & VK_SKEL_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, entry, "skeleton")) return rc;
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    if (n > kDistMaxVoxels) return fail(ctx, VK_ERR_UNSUPPORTED, "skeleton: a volume of more than 2^32 - 2 voxels (voxel indices are 32-bit)");

    const FilterGrid F = filter_grid(ctx->nx, ctx->ny, ctx->nz, kLabelTile, ctx->skel_max_blocks);
    SkelDesc G{};
    G.nx = ctx->nx; G.ny = ctx->ny; G.nz = ctx->nz;
    G.curve = req->mode == (uint32_t)VK_SKEL_CURVE ? 1u : 0u;
    G.ntx = F.ntx; G.nty = F.nty; G.ntz = F.ntz;
    G.tiles = (uint32_t)F.tiles;
    G.box = B;
    G.lo_k = label_scale_bound(req->lo, ctx->format); G.hi_k = label_scale_bound(req->hi, ctx->format);
    G.fill_in_on = (req->flags & VK_SKEL_FILL_IN) ? 1u : 0u;
    G.fill_in_bits = G.fill_in_on ? label_fill_bits(req->fill_in, ctx->format) : 0u;
    G.fill_out_bits = label_fill_bits(req->fill_out, ctx->format);
    G.n = n;
    const uint32_t tile_blocks = F.blocks;
    const uint32_t seed_blocks = std::min<uint32_t>(tile_blocks, kPassMaxPartials);  // a partial result per workgroup
    const uint32_t voxel_blocks = std::min<uint32_t>(label_blocks((n + kSkelVoxelThreads - 1u) / kSkelVoxelThreads, ctx->skel_max_blocks), kPassMaxPartials);

    const int kind = ctx->vol_kind;
    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, entry};
    hipError_t &e = call.e;
    // (debug, vk_debug_set_param("skel_timing", k): phase k alone between the context's timer events, read with vk_timer_elapsed_ms --
    //  1 seed, 2 thin (every sub-pass of every iteration, with the host's looks at the counts), 3 stats (with the classes), 4 dense;
    //  9: nothing is timed, and a call that succeeds leaves "skeleton: iterations I launches L visits V deleted D" as the context's last
    //  message)
    const uint32_t timing = ctx->skel_timing;

    const size_t dense_bytes = pass_dense_bytes(ctx->format, n);
    DeviceTemp d_state, d_marks, d_counts, d_seed, d_partial, d_class, d_out;
    if (int rc = call.alloc(d_state, (size_t)n, "the state bytes")) return rc;
    if (int rc = call.alloc(d_marks, (size_t)G.tiles * 8u, "the tile stamps")) return rc;
    if (int rc = call.alloc(d_counts, (size_t)kSkelBatch * kSkelIterWords * 8u, "the iterations' counts")) return rc;
    PassPartials seeds(seed_blocks, 1u), sums(voxel_blocks, kSkelStatsWords);
    if (int rc = call.alloc(d_seed, seeds.bytes(), "the partial totals")) return rc;
    if (int rc = call.alloc(d_partial, sums.bytes(), "the partial totals")) return rc;
    if (class_out)
        if (int rc = call.alloc(d_class, (size_t)n, "the classes")) return rc;
    if (dense_out || install)
        if (int rc = call.alloc(d_out, dense_bytes, "the output buffer")) return rc;
    uint8_t *state = (uint8_t *)d_state.p;
    uint32_t *marks[2] = {(uint32_t *)d_marks.p, (uint32_t *)d_marks.p + G.tiles};
    unsigned long long *counts = (unsigned long long *)d_counts.p;

    call.phase(timing == 1u, [&] {
        e = hipMemsetAsync(d_marks.p, 0, (size_t)G.tiles * 8u, ctx->stream);  // iteration numbers start at 1
        if (e != hipSuccess) return;
        with_scalar_kind(kind, [&](auto VOL) {
            hipLaunchKernelGGL(skel_seed_kernel<VOL()>, dim3(seed_blocks), dim3(kLabelThreads), 0, ctx->stream, V, G, state, marks[1], (unsigned long long *)d_seed.p);
        });
    });

    // The iterations, whole ones in batches (PassCall::iterate), max_iterations of them at most.  An iteration that deletes nothing stamps
    // no tile, so the iterations behind it in its batch exit at once and the state is the fixed point when the batch is over.
    unsigned long long iterations = 0ull, launches = 0ull, visits = 0ull, deleted = 0ull;
    uint32_t converged = 0u;
    call.iterate<kSkelBatch, kSkelIterWords>(timing == 2u, counts, req->max_iterations,
        [&](uint32_t r, unsigned long long *slot) {
            const uint32_t it = r + 1u;
            G.iteration = it;
            for (uint32_t s = 0; s < 8u; s++)
                call.enqueue([&] {
                    G.subpass = s;
                    hipLaunchKernelGGL(skel_thin_kernel, dim3(tile_blocks), dim3(kLabelThreads), 0, ctx->stream, G, state, (const uint32_t *)marks[it & 1u], marks[(it + 1u) & 1u], slot);
                    launches++;
                });
        },
        [&](const unsigned long long *c) {
            visits += c[1]; deleted += c[0];
            if (c[0]) iterations++;
            else converged = 1u;
            return c[0] == 0ull;
        });

    call.phase(timing == 3u, [&] {
        hipLaunchKernelGGL(skel_stats_kernel, dim3(voxel_blocks), dim3(kSkelVoxelThreads), 0, ctx->stream, G, (const uint8_t *)state, (uint8_t *)d_class.p, (unsigned long long *)d_partial.p);
    });
    seeds.download(call, d_seed.p);
    sums.download(call, d_partial.p);
    call.download(class_out, d_class.p, (size_t)n);
    if (dense_out || install) {
        call.phase(timing == 4u, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(skel_dense_kernel<VOL()>, dim3(voxel_blocks), dim3(kSkelVoxelThreads), 0, ctx->stream, V, G, (const uint8_t *)state, d_out.p);
            });
        });
        call.download(dense_out, d_out.p, dense_bytes);
    }
    if (int rc = call.finish()) return rc;

    vk_skeleton_result r{};
    r.n_foreground = seeds.sum(0u);
    r.n_skeleton = sums.sum(0u); r.n_isolated = sums.sum(1u); r.n_end = sums.sum(2u); r.n_regular = sums.sum(3u); r.n_junction = sums.sum(4u);
    for (uint32_t j = 0; j < (uint32_t)VK_SKEL_LINKS; j++) r.links[j] = sums.sum(5u + j);
    r.iterations = (uint32_t)iterations;
    r.converged = converged;
    if (result) *result = r;
    const int rc = install ? call.install(d_out, G.nx, G.ny, G.nz, ctx->format, ctx->layout) : VK_OK;
    if (rc == VK_OK && timing == 9u)
        ctx->err = "skeleton: iterations " + std::to_string(iterations) + " launches " + std::to_string(launches) + " visits " + std::to_string(visits) + " deleted " + std::to_string(deleted);
    return rc;
}

}  // extern "C"
