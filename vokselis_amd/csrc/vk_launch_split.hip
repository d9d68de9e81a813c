// vk_launch_split.hip -- split touching objects (vk_split_components): S is eroded by a radius, what survives is
// labelled as markers, the markers grow back over S round by round, what no marker reaches is labelled on its own, and S is cut where
// two regions meet.  The request's validation, the states of the growth array and a voxel's step of a round are vk_split.hpp's, shared
// with the host fuzz.  The distance kernels (vk_dist_launch.hpp) and the label pass's tile / seam / flatten / scan / number / stats
// kernels (vk_label_launch.hpp) are borrowed as they are; the kernels here are the growth's and the cut's.
//
//   distance  D2(not S, .): the distance pass's first round.
//   markers   tile (predicate: D2 > R2, from the word array), seam, flatten: every voxel of K holds its marker component's anchor.
//   seed      the state array: K keeps its anchors, S \ K becomes kSplitUnreached, everything else stays kLabelBackground.
//   grow      one launch per round, from one state array into the other: a voxel that is unreached takes the smallest anchor among its
//             neighbours in the array the round before left, every other voxel is copied.  The host launches kSplitBatch rounds, reads
//             how many voxels each labelled, and stops after the batch in which a round labelled none.
//   residue   tile (predicate: state == kSplitUnreached), seam, flatten over what no marker reached.
//   merge     a reached voxel's parent is its anchor, an unreached one's its residue root: one parent array in which a root is a
//             region's anchor; roots and foreground voxels are counted per chunk for the scan.
//   number, stats   the label pass's, over the merged array.
//   cut       one kernel per volume kind: the label, the neighbours' labels, then the stored texel or the fill; n_cut as one partial sum
//             per workgroup.
// Phases and rounds are separated by kernel boundaries: no flags, tickets or grid barriers, no wave waits for another workgroup, and no
// kernel here reads an address that another thread of the same launch writes.  Plain C++; no inline assembly.
#include "vk_dist_launch.hpp"
#include "vk_label_launch.hpp"
#include "vk_pass_blocks.hpp"
#include "vk_split.hpp"
#include "vk_texel.hpp"

#include <utility>

using namespace vk;

struct SplitPlainLoad {
    static __device__ __forceinline__ uint32_t load(const uint32_t *p, uint32_t i) { return p[i]; }
};

// state is the markers' flattened parent array on entry: an anchor on K, kLabelBackground elsewhere.  d2 != 0 exactly on S.
__global__ __launch_bounds__(kLabelThreads) void split_seed_kernel(const LabelDesc D, const uint32_t *__restrict__ d2, uint32_t *__restrict__ state) {
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;
            if (i < D.n && state[i] == kLabelBackground && d2[i] != 0u) state[i] = kSplitUnreached;
        }
    }
}

// One round: out = in, but an unreached voxel takes the smallest anchor beside it in `in`.  *labelled: the voxels this round labelled.
__global__ __launch_bounds__(kLabelThreads) void split_grow_kernel(const LabelDesc D, const uint32_t *__restrict__ in, uint32_t *__restrict__ out, unsigned long long *labelled) {
    __shared__ unsigned long long s_n;
    if (threadIdx.x == 0) s_n = 0ull;
    __syncthreads();
    uint32_t mine = 0u;
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;
            if (i >= D.n) continue;
            uint32_t s = in[i];
            if (s == kSplitUnreached) {
                uint32_t x, y, z;
                label_coords((uint32_t)i, D.nx, D.ny, x, y, z);
                s = split_grow_voxel<SplitPlainLoad>(in, x, y, z, D.nx, D.ny, D.nz, D.conn_sum);
                mine += s != kSplitUnreached;
            }
            out[i] = s;
        }
    }
    block_add(&s_n, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(labelled, s_n);  // integers: the order of the adds does not show
}

// parent is the residue's flattened parent array on entry (a root on the unreached voxels, kLabelBackground elsewhere) and the merged one
// on exit: a reached voxel holds its anchor.  A root of the merged array is a voxel that holds its own index.
__global__ __launch_bounds__(kLabelThreads) void split_merge_kernel(const LabelDesc D, const uint32_t *__restrict__ state, uint32_t *__restrict__ parent, uint32_t *__restrict__ chunk_roots,
                                                                    uint32_t *__restrict__ chunk_fg) {
    __shared__ unsigned long long s_roots, s_fg;
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {  // block-uniform
        if (threadIdx.x == 0) { s_roots = 0ull; s_fg = 0ull; }
        __syncthreads();
        uint32_t roots = 0u, fg = 0u;
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;
            if (i >= D.n) continue;
            const uint32_t s = state[i];
            const uint32_t p = s < kSplitUnreached ? s : parent[i];
            if (s < kSplitUnreached) parent[i] = p;
            fg += p != kLabelBackground;
            roots += p == (uint32_t)i;
        }
        block_add(&s_roots, roots);
        block_add(&s_fg, fg);
        __syncthreads();
        if (threadIdx.x == 0) { chunk_roots[chunk] = (uint32_t)s_roots; chunk_fg[chunk] = (uint32_t)s_fg; }
        __syncthreads();
    }
}

// out (may be NULL): the stored texel, or the fill where a neighbour in S carries a smaller id.  partial[b]: the cut voxels workgroup b saw.
template <int VOL>
__global__ __launch_bounds__(kLabelThreads) void split_cut_kernel(const VolumeDesc V, const LabelDesc D, const uint32_t *__restrict__ labels, void *__restrict__ out,
                                                                  unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n;
    if (threadIdx.x == 0) s_n = 0ull;
    __syncthreads();
    uint32_t mine = 0u;
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;
            if (i >= D.n) continue;
            uint32_t x, y, z;
            label_coords((uint32_t)i, D.nx, D.ny, x, y, z);
            const uint32_t id = labels[i];
            bool cut = false;
            if (id > 1u) {  // region 1 has no smaller id beside it
                for (uint32_t o = 0; o < kLabelOffsets; o++) {
                    int dx, dy, dz;
                    label_offset(o, dx, dy, dz);
                    if (!label_adjacent(dx, dy, dz, D.conn_sum)) continue;
                    const int64_t hx = (int64_t)x + dx, hy = (int64_t)y + dy, hz = (int64_t)z + dz;  // no wrap
                    if (hx < 0 || hy < 0 || hz < 0 || hx >= (int64_t)D.nx || hy >= (int64_t)D.ny || hz >= (int64_t)D.nz) continue;
                    const uint32_t other = labels[voxel_index((uint32_t)hx, (uint32_t)hy, (uint32_t)hz, D.nx, D.ny)];
                    cut = cut || (other != 0u && other < id);
                }
            }
            mine += cut;
            if (!out) continue;
            const uint32_t bits = cut ? D.fill_bits : voxel_texel_bits<VOL>(V, x, y, z);
            store_texel_bits<texel_class(VOL)>(out, i, bits);
        }
    }
    block_add(&s_n, mine);
    publish_partials<1u>(partial, &s_n);
}

extern "C" {

int vk_split_components(vk_ctx *ctx, const vk_split_request *req, const vk_voxel_box *box, uint32_t *labels_out, vk_component *components, uint64_t cap_components, void *dense_out,
                        vk_split_result *result) {
    static const char *const entry = "vk_split_components";
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = split_validate(req, labels_out != nullptr, components != nullptr, cap_components, dense_out != nullptr, result != nullptr))
        return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + why);
    const bool install = (req->flags & VK_SPLIT_INSTALL) != 0u;
    if (int rc = pass_install_refused(ctx, entry, "VK_SPLIT_INSTALL", install)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, entry, "split")) return rc;
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, entry, "VK_SPLIT_CLIP_BOX", box, (req->flags & VK_SPLIT_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, entry, "split")) return rc;
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    if (!label_volume_fits(ctx->nx, ctx->ny, ctx->nz)) return fail(ctx, VK_ERR_UNSUPPORTED, "split: a volume of more than 2^32 - 2 voxels (labels are 32-bit)");
    if (!dist_d2_fits(req->spacing, ctx->nx, ctx->ny, ctx->nz))
        return fail(ctx, VK_ERR_UNSUPPORTED, "split: sum_c (spacing[c] (n_c - 1))^2 exceeds 0xFFFFFFFE: a squared distance would not fit in 32 bits");
    const float lo_k = label_scale_bound(req->lo, ctx->format), hi_k = label_scale_bound(req->hi, ctx->format);
    if ((dense_out || install) && !split_fill_leaves_set(req->fill_out, ctx->format, lo_k, hi_k))
        return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": fill_out, once stored, lies inside [lo, hi]: the cut would cut nothing");

    const int kind = ctx->vol_kind;
    const FilterGrid G = filter_grid(ctx->nx, ctx->ny, ctx->nz, kLabelTile, ctx->label_max_blocks);
    LabelDesc D{};
    D.nx = ctx->nx; D.ny = ctx->ny; D.nz = ctx->nz;
    D.conn_sum = label_conn_sum(req->connectivity);
    D.box = B;
    D.ntx = G.ntx; D.nty = G.nty; D.tiles = G.tiles;
    D.n = n;
    D.chunks = label_chunks(n);
    D.lo_k = lo_k; D.hi_k = hi_k;
    D.fill_bits = label_fill_bits(req->fill_out, ctx->format);
    const uint32_t chunk_blocks = label_blocks(D.chunks, ctx->label_max_blocks);
    const uint32_t cut_blocks = std::min(chunk_blocks, kPassMaxPartials);  // the cut kernel's grid: one partial sum per workgroup
    const uint64_t r2 = dist_r2(req->radius);  // <= VK_DIST_MAX_RADIUS^2 < VK_DIST_INF: r2 + 1 fits in a word

    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, entry};
    // (debug, vk_debug_set_param("split_timing", k): phase k alone between the context's timer events, read with vk_timer_elapsed_ms --
    //  1 distance, 2 markers, 3 growth (every round, with the host's looks at the counts), 4 residue, 5 merge, 6 number and stats, 7 cut)
    const uint32_t timing = ctx->split_timing;

    DeviceTemp d_a, d_b, d_c, d_chunk_roots, d_chunk_fg, d_totals, d_counts, d_partial;
    if (int rc = call.alloc(d_a, (size_t)n * 4u, "the distance array")) return rc;
    if (int rc = call.alloc(d_b, (size_t)n * 4u, "the state array")) return rc;
    if (int rc = call.alloc(d_c, (size_t)n * 4u, "the second state array")) return rc;
    if (int rc = call.alloc(d_chunk_roots, (size_t)D.chunks * 4u, "the chunk counts")) return rc;
    if (int rc = call.alloc(d_chunk_fg, (size_t)D.chunks * 4u, "the chunk counts")) return rc;
    if (int rc = call.alloc(d_totals, 48u, "the totals")) return rc;
    if (int rc = call.alloc(d_counts, (size_t)kSplitBatch * 8u, "the rounds' counts")) return rc;
    PassPartials sums(cut_blocks, 1u);
    if (int rc = call.alloc(d_partial, sums.bytes(), "the partial counts")) return rc;
    uint32_t *a = (uint32_t *)d_a.p, *chunk_roots = (uint32_t *)d_chunk_roots.p, *chunk_fg = (uint32_t *)d_chunk_fg.p;
    unsigned long long *d_tot = (unsigned long long *)d_totals.p, *counts = (unsigned long long *)d_counts.p;

    // D2(not S, .) into a; the markers' parent array into b
    call.phase(timing == 1u, [&] { dist_launch_inside(ctx, B, lo_k, hi_k, req->spacing, a, (uint32_t *)d_b.p, (uint32_t *)d_c.p); });
    uint32_t *cur = (uint32_t *)d_b.p, *other = (uint32_t *)d_c.p;
    call.phase(timing == 2u, [&] {
        label_launch_tile_words(ctx->stream, G.blocks, D, LabelWords{a, (uint32_t)(r2 + 1u), 0xffffffffu}, cur);
        label_launch_seam(ctx->stream, G.blocks, D, cur);
        label_launch_flatten(ctx->stream, chunk_blocks, D, cur, chunk_roots, chunk_fg);
        label_launch_scan(ctx->stream, D.chunks, chunk_roots, chunk_fg, d_tot);  // {marker components, |K|}
        hipLaunchKernelGGL(split_seed_kernel, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, D, (const uint32_t *)a, cur);
    });

    // The growth (PassCall::iterate).  Every batch but the last labels at least one voxel in each of its rounds, and S is finite: the loop
    // ends.  A round that labels nothing copies the state, and so does every round after it: `cur` holds the fixed point when the batch is over.
    uint32_t rounds = 0u;
    call.iterate<kSplitBatch, 1u>(timing == 3u, counts, 0u,
        [&](uint32_t, unsigned long long *slot) {
            hipLaunchKernelGGL(split_grow_kernel, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, D, (const uint32_t *)cur, other, slot);
            std::swap(cur, other);
        },
        [&](const unsigned long long *c) {
            if (c[0]) rounds++;
            return c[0] == 0ull;
        });

    // what no marker reached, labelled on its own into `other`; then the merged parent array, in place
    call.phase(timing == 4u, [&] {
        label_launch_tile_words(ctx->stream, G.blocks, D, LabelWords{cur, kSplitUnreached, kSplitUnreached}, other);
        label_launch_seam(ctx->stream, G.blocks, D, other);
        label_launch_flatten(ctx->stream, chunk_blocks, D, other, chunk_roots, chunk_fg);
        label_launch_scan(ctx->stream, D.chunks, chunk_roots, chunk_fg, d_tot + 2);  // {residue regions, residue voxels}
    });
    uint32_t *parent = other, *labels = a;  // D2 is not needed any more
    unsigned long long totals[6] = {};
    call.phase(timing == 5u, [&] {
        hipLaunchKernelGGL(split_merge_kernel, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, D, (const uint32_t *)cur, parent, chunk_roots, chunk_fg);
        label_launch_scan(ctx->stream, D.chunks, chunk_roots, chunk_fg, d_tot + 4);  // {regions, |S|}
    });
    call.download(totals, d_tot, sizeof totals);
    if (int rc = call.finish()) return rc;
    const uint64_t n_reg = totals[4];

    DeviceTemp d_first, d_size, d_box;
    if (int rc = call.alloc(d_first, (size_t)n_reg * 4u, "the region records")) return rc;
    if (int rc = call.alloc(d_size, (size_t)n_reg * 4u, "the region records")) return rc;
    if (int rc = call.alloc(d_box, (size_t)n_reg * 24u, "the region records")) return rc;
    const LabelRecords R{(uint32_t *)d_first.p, (uint32_t *)d_size.p, (uint32_t *)d_box.p};
    call.phase(timing == 6u, [&] {
        if (n_reg) label_launch_number(ctx->stream, chunk_blocks, D, parent, chunk_roots, labels, R);
        label_launch_stats(ctx->stream, chunk_blocks, D, parent, labels, R);
    });

    const size_t dense_bytes = pass_dense_bytes(ctx->format, n);
    DeviceTemp d_out;
    if (dense_out || install)
        if (int rc = call.alloc(d_out, dense_bytes, "the output buffer")) return rc;
    if (dense_out || install || result) {
        call.phase(timing == 7u, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(split_cut_kernel<VOL()>, dim3(cut_blocks), dim3(kLabelThreads), 0, ctx->stream, V, D, (const uint32_t *)labels, d_out.p, (unsigned long long *)d_partial.p);
            });
        });
        sums.download(call, d_partial.p);
        call.download(dense_out, d_out.p, dense_bytes);
    }
    call.download(labels_out, labels, (size_t)n * 4u);
    const uint64_t n_rec = components ? (n_reg < cap_components ? n_reg : cap_components) : 0u;
    if (int rc = label_download_components(call, R, nullptr, n_rec, components)) return rc;
    if (result) {
        vk_split_result r{};
        r.n_regions = n_reg; r.n_foreground = totals[5];
        r.n_markers = totals[0]; r.n_marker_voxels = totals[1];
        r.n_residue_regions = totals[2]; r.n_residue_voxels = totals[3];
        r.n_cut = sums.sum(0u);
        r.rounds = rounds;
        *result = r;
    }
    return install ? call.install(d_out, D.nx, D.ny, D.nz, ctx->format, ctx->layout) : VK_OK;
}

}  // extern "C"
