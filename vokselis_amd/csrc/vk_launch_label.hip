// vk_launch_label.hip -- connected components of a value range (vk_label_components): a union-find over the whole
// volume in which a root is always the smallest linear index of its set.  The predicate, the neighbour offsets, find and union, the
// tile, seam and chunk arithmetic, the selection and the request's validation are vk_label.hpp's, shared with the host fuzz.
//
//   tile     one kernel per volume kind.  A workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ...: it loads the tile's predicate
//            through vk_texel.hpp (no halo), unites every voxel with its earlier neighbours inside the tile by LDS atomics between two
//            barriers, and writes each voxel's tile-local root as a global index (background: kLabelBackground) -- the whole parent array.
//   seam     every voxel on a tile's low faces is united with its neighbours in earlier tiles: the only kernel whose workgroups talk to
//            each other.  Every read of the parent array is an agent-scope atomic load, every write an agent-scope atomic min.
//   flatten  each voxel's parent becomes its root; roots and foreground voxels are counted per chunk.
//   scan     the chunk counts become exclusive offsets (one workgroup).
//   number   roots take their ids in index order and initialise their component's record.
//   label    every voxel takes its root's id; sizes and bounding boxes are gathered by integer atomics: lanes of a wave that share a
//            root and a row are combined first, their sums meet in a table in LDS, and one add per component and chunk goes to memory.
//   mask     one kernel per volume kind: label, keep byte, then the stored texel or the fill.
// Phases are separated by kernel boundaries: no flags, tickets or grid barriers, and no wave ever waits for another workgroup.  Every
// loop whose trip count depends on data names what decreases.  Loop bounds are block-uniform wherever a barrier stands.  Plain C++;
// no inline assembly.  wave64 is assumed in label_stats_kernel alone (the ballot is 64 bits wide).
// The tile kernel's body, label_tile, takes its predicate as a parameter: the volume's texels here, a word array for the split pass, which
// borrows the other kernels as they are through the launchers at the end (vk_label_launch.hpp).
#include "vk_label_launch.hpp"
#include "vk_texel.hpp"

#include <vector>

using namespace vk;

static_assert(sizeof(LabelDesc) % 8 == 0 && pass_kernargs_fit<LabelDesc>, "label kernels: VolumeDesc + LabelDesc");

// the parent array in LDS, shared by the waves of a workgroup between two barriers
struct LdsParent {
    static __device__ __forceinline__ uint32_t load(uint32_t *p, uint32_t i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ __forceinline__ uint32_t fetch_min(uint32_t *p, uint32_t i, uint32_t v) { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
// ... and in global memory, shared by every workgroup of the launch: agent scope (the loads pass the CU's L1 by, the min runs in memory's own atomic unit)
struct GlobalParent {
    static __device__ __forceinline__ uint32_t load(uint32_t *p, uint32_t i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint32_t fetch_min(uint32_t *p, uint32_t i, uint32_t v) { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// Where a tile's predicate comes from: the volume's stored texel against [lo_k, hi_k] inside the box, or a word array against [lo, hi]
// (vk_label_launch.hpp: the split pass's markers and residue).  Called for voxels inside the volume only.
template <int VOL>
struct LabelVolumePredicate {
    const VolumeDesc V;
    __device__ __forceinline__ bool operator()(const LabelDesc &D, uint32_t gx, uint32_t gy, uint32_t gz) const {
        return label_in_box(gx, gy, gz, D.box) && label_foreground(texel_f32<VOL>(voxel_texel_bits<VOL>(V, gx, gy, gz)), D.lo_k, D.hi_k);
    }
};
struct LabelWordsPredicate {
    const LabelWords W;
    __device__ __forceinline__ bool operator()(const LabelDesc &D, uint32_t gx, uint32_t gy, uint32_t gz) const {
        const uint32_t w = W.w[voxel_index(gx, gy, gz, D.nx, D.ny)];
        return w >= W.lo && w <= W.hi;
    }
};

template <class PRED>
__device__ __forceinline__ void label_tile(const PRED pred, const LabelDesc D, uint32_t *__restrict__ parent) {
    __shared__ uint32_t lds[kLabelTileVoxels];
    for (uint64_t tile = blockIdx.x; tile < D.tiles; tile += gridDim.x) {  // block-uniform
        uint32_t x0, y0, z0;
        filter_tile_origin(tile, D.ntx, D.nty, kLabelTile, x0, y0, z0);
        for (uint32_t k = 0; k < kLabelPerThread; k++) {
            const uint32_t e = threadIdx.x + k * kLabelThreads;
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            bool fg = false;
            if (gx < D.nx && gy < D.ny && gz < D.nz) fg = pred(D, gx, gy, gz);
            lds[e] = fg ? e : kLabelBackground;
        }
        __syncthreads();
        // whether an element is background never changes from here on; its parent does
        for (uint32_t k = 0; k < kLabelPerThread; k++) {
            const uint32_t e = threadIdx.x + k * kLabelThreads;
            if (LdsParent::load(lds, e) == kLabelBackground) continue;
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            for (uint32_t o = 0; o < kLabelCentre; o++) {  // the neighbours that come earlier
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                if (!label_adjacent(dx, dy, dz, D.conn_sum) || !label_in_tile((int)lx + dx, (int)ly + dy, (int)lz + dz)) continue;
                const uint32_t ne = label_local_index(lx + dx, ly + dy, lz + dz);
                if (LdsParent::load(lds, ne) != kLabelBackground) label_union<LdsParent>(lds, e, ne);
            }
        }
        __syncthreads();
        for (uint32_t k = 0; k < kLabelPerThread; k++) {
            const uint32_t e = threadIdx.x + k * kLabelThreads;
            uint32_t lx, ly, lz;
            label_local_coords(e, lx, ly, lz);
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            if (gx >= D.nx || gy >= D.ny || gz >= D.nz) continue;
            uint32_t root = kLabelBackground;
            if (lds[e] != kLabelBackground) {
                uint32_t rx, ry, rz;
                label_local_coords(label_find<LdsParent>(lds, e), rx, ry, rz);  // a foreground voxel: inside the volume
                root = (uint32_t)voxel_index(x0 + rx, y0 + ry, z0 + rz, D.nx, D.ny);
            }
            parent[voxel_index(gx, gy, gz, D.nx, D.ny)] = root;
        }
        __syncthreads();  // the next tile's load overwrites the labels
    }
}

template <int VOL>
__global__ __launch_bounds__(kLabelThreads) void label_tile_kernel(const VolumeDesc V, const LabelDesc D, uint32_t *__restrict__ parent) {
    label_tile(LabelVolumePredicate<VOL>{V}, D, parent);
}
__global__ __launch_bounds__(kLabelThreads) void label_tile_words_kernel(const LabelWords W, const LabelDesc D, uint32_t *__restrict__ parent) {
    label_tile(LabelWordsPredicate{W}, D, parent);
}

__global__ __launch_bounds__(kLabelThreads) void label_seam_kernel(const LabelDesc D, uint32_t *parent) {
    for (uint64_t tile = blockIdx.x; tile < D.tiles; tile += gridDim.x) {
        uint32_t x0, y0, z0;
        filter_tile_origin(tile, D.ntx, D.nty, kLabelTile, x0, y0, z0);
        for (uint32_t e = threadIdx.x; e < kLabelSeamVoxels; e += kLabelThreads) {
            uint32_t lx, ly, lz;
            label_seam_voxel(e, lx, ly, lz);
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            if (gx >= D.nx || gy >= D.ny || gz >= D.nz) continue;
            const uint32_t i = (uint32_t)voxel_index(gx, gy, gz, D.nx, D.ny);
            if (GlobalParent::load(parent, i) == kLabelBackground) continue;
            for (uint32_t o = 0; o < kLabelOffsets; o++) {
                int dx, dy, dz;
                label_offset(o, dx, dy, dz);
                if (!label_adjacent(dx, dy, dz, D.conn_sum) || !label_seam_owner(lx, ly, lz, dx, dy, dz)) continue;
                const int64_t hx = (int64_t)gx + dx, hy = (int64_t)gy + dy, hz = (int64_t)gz + dz;  // no wrap: a neighbour outside the volume does not exist
                if (hx < 0 || hy < 0 || hz < 0 || hx >= (int64_t)D.nx || hy >= (int64_t)D.ny || hz >= (int64_t)D.nz) continue;
                const uint32_t j = (uint32_t)voxel_index((uint32_t)hx, (uint32_t)hy, (uint32_t)hz, D.nx, D.ny);
                if (GlobalParent::load(parent, j) != kLabelBackground) label_union<GlobalParent>(parent, i, j);
            }
        }
    }
}

// Every voxel's parent becomes its root, in place.  Another workgroup's walk may pass through a voxel while its parent is replaced: it
// reads the old parent or the root, an ancestor either way, and a root's own entry is never written here.
__global__ __launch_bounds__(kLabelThreads) void label_flatten_kernel(const LabelDesc D, uint32_t *parent, uint32_t *__restrict__ chunk_roots, uint32_t *__restrict__ chunk_fg) {
    __shared__ uint32_t s_roots, s_fg;
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {  // block-uniform
        if (threadIdx.x == 0) { s_roots = 0u; s_fg = 0u; }
        __syncthreads();
        uint32_t roots = 0u, fg = 0u;
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;
            if (i >= D.n || GlobalParent::load(parent, (uint32_t)i) == kLabelBackground) continue;
            fg++;
            const uint32_t r = label_find<GlobalParent>(parent, (uint32_t)i);
            if (r == (uint32_t)i) roots++;
            else __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (roots) atomicAdd(&s_roots, roots);
        if (fg) atomicAdd(&s_fg, fg);
        __syncthreads();
        if (threadIdx.x == 0) { chunk_roots[chunk] = s_roots; chunk_fg[chunk] = s_fg; }
        __syncthreads();
    }
}

// the inclusive sum of v over the threads of a workgroup up to and including this one; total: over all of them.  s: kLabelThreads words of LDS.
__device__ __forceinline__ uint32_t label_block_scan(uint32_t *s, uint32_t v, uint32_t &total) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kLabelThreads; d <<= 1) {
        const uint32_t t = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    const uint32_t inc = s[threadIdx.x];
    total = s[kLabelThreads - 1u];
    __syncthreads();  // s is free again
    return inc;
}

// chunk_roots becomes its exclusive scan; totals = {components, foreground voxels}.  One workgroup.
__global__ __launch_bounds__(kLabelThreads) void label_scan_kernel(uint32_t chunks, uint32_t *__restrict__ chunk_roots, const uint32_t *__restrict__ chunk_fg, unsigned long long *__restrict__ totals) {
    __shared__ uint32_t s[kLabelThreads];
    __shared__ unsigned long long s_fg;
    if (threadIdx.x == 0) s_fg = 0ull;
    uint32_t carry = 0u;
    unsigned long long fg = 0ull;
    for (uint32_t base = 0; base < chunks; base += kLabelThreads) {  // block-uniform
        const uint32_t c = base + threadIdx.x;
        const uint32_t v = c < chunks ? chunk_roots[c] : 0u;
        if (c < chunks) fg += chunk_fg[c];
        uint32_t total;
        const uint32_t inc = label_block_scan(s, v, total);
        if (c < chunks) chunk_roots[c] = carry + inc - v;
        carry += total;
    }
    __syncthreads();
    if (fg) atomicAdd(&s_fg, fg);
    __syncthreads();
    if (threadIdx.x == 0) { totals[0] = carry; totals[1] = s_fg; }
}

// Roots take their ids, 1 + the exclusive scan of the root flags in index order: a thread holds 16 consecutive voxels.
__global__ __launch_bounds__(kLabelThreads) void label_number_kernel(const LabelDesc D, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ chunk_offset, uint32_t *__restrict__ labels,
                                                                     const LabelRecords R) {
    __shared__ uint32_t s[kLabelThreads];
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {  // block-uniform
        const uint64_t i0 = (uint64_t)chunk * kLabelChunk + (uint64_t)threadIdx.x * kLabelChunkPerThread;
        uint32_t mask = 0u;
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++)
            if (i0 + k < D.n && parent[i0 + k] == (uint32_t)(i0 + k)) mask |= 1u << k;
        const uint32_t cnt = (uint32_t)__popc(mask);
        uint32_t total;
        uint32_t id = chunk_offset[chunk] + label_block_scan(s, cnt, total) - cnt + 1u;
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            if (!(mask & (1u << k))) continue;
            const uint32_t c = id - 1u;
            labels[i0 + k] = id++;
            R.first[c] = (uint32_t)(i0 + k);
            R.size[c] = 0u;
            for (uint32_t a = 0; a < 6u; a++) R.box[6u * (size_t)c + a] = a < 3u ? 0xffffffffu : 0u;
        }
    }
}

// lowers / raises a bound of a box only where a look at it says it may have to move: the look may be stale, that is an older and
// so a looser bound, which costs an atomic and never a result
__device__ __forceinline__ void label_box_min(uint32_t *p, uint32_t v) { if (v < *p) atomicMin(p, v); }
__device__ __forceinline__ void label_box_max(uint32_t *p, uint32_t v) { if (v > *p) atomicMax(p, v); }

// Every voxel takes its root's id (0: background); sizes and boxes are gathered in two steps.  wave64.  A run is a stretch of consecutive
// lanes -- consecutive voxels -- with one id in one row: its head lane alone adds the run's length and its extent in x.  It adds them
// to the workgroup's table in LDS, kLabelSlots entries found by a hash of the id with no probing: the first id to ask owns a slot
// until the chunk ends, an id that finds its slot taken goes to memory directly.  After the chunk one thread per used slot sends the sums
// on.  A volume that is one component sends one add per 4096 voxels to the one address, not one per lane or run: the adds of a chunk
// meet in LDS, where they cost a few cycles each, and every sum is of integers, so the order does not show.
constexpr uint32_t kLabelSlots = 512;
__device__ __forceinline__ uint32_t label_slot(uint32_t id) { return (id * 2654435761u) >> 23; }  // the top 9 bits of a multiplicative hash
static_assert(kLabelSlots == 1u << 9 && kLabelSlots % kLabelThreads == 0, "label_slot yields 9 bits; the flush takes whole passes");

__global__ __launch_bounds__(kLabelThreads) void label_stats_kernel(const LabelDesc D, const uint32_t *__restrict__ parent, uint32_t *labels, const LabelRecords R) {
    __shared__ uint32_t s_key[kLabelSlots], s_cnt[kLabelSlots], s_box[6][kLabelSlots];
    for (uint32_t s = threadIdx.x; s < kLabelSlots; s += kLabelThreads) {
        s_key[s] = 0u; s_cnt[s] = 0u;
        for (uint32_t a = 0; a < 6u; a++) s_box[a][s] = a < 3u ? 0xffffffffu : 0u;
    }
    __syncthreads();
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {  // block-uniform
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;  // a wave: 64 consecutive voxels
            uint32_t id = 0u, x = 0u, y = 0u, z = 0u;
            if (i < D.n) {
                const uint32_t r = parent[i];
                // a root's label is the number kernel's and is not written here; every other voxel writes its own: no address is both read and written
                if (r != kLabelBackground) id = labels[r];
                if (r != (uint32_t)i) labels[i] = id;
                label_coords((uint32_t)i, D.nx, D.ny, x, y, z);
            }
            const uint32_t lane = threadIdx.x & 63u;
            const uint32_t prev = (uint32_t)__shfl_up((int)id, 1);
            const bool boundary = lane == 0u || prev != id || x == 0u;  // a run starts here (of a component, or of background)
            const unsigned long long starts = __ballot(boundary);
            if (id != 0u && boundary) {
                const unsigned long long after = lane == 63u ? 0ull : starts >> (lane + 1u);
                const uint32_t len = after ? (uint32_t)__ffsll(after) : 64u - lane;  // to the next start, or to the wave's end
                const uint32_t slot = label_slot(id);
                const uint32_t owner = atomicCAS(&s_key[slot], 0u, id);
                if (owner == 0u || owner == id) {
                    atomicAdd(&s_cnt[slot], len);
                    atomicMin(&s_box[0][slot], x); atomicMin(&s_box[1][slot], y); atomicMin(&s_box[2][slot], z);
                    atomicMax(&s_box[3][slot], x + len - 1u); atomicMax(&s_box[4][slot], y); atomicMax(&s_box[5][slot], z);
                } else {
                    const uint32_t c = id - 1u;
                    atomicAdd(R.size + c, len);
                    uint32_t *b = R.box + 6u * (size_t)c;
                    label_box_min(b + 0, x); label_box_min(b + 1, y); label_box_min(b + 2, z);
                    label_box_max(b + 3, x + len - 1u); label_box_max(b + 4, y); label_box_max(b + 5, z);
                }
            }
        }
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < kLabelSlots; s += kLabelThreads) {
            const uint32_t id = s_key[s];
            if (id == 0u) continue;
            const uint32_t c = id - 1u;
            atomicAdd(R.size + c, s_cnt[s]);
            uint32_t *b = R.box + 6u * (size_t)c;
            for (uint32_t a = 0; a < 3u; a++) { label_box_min(b + a, s_box[a][s]); label_box_max(b + 3u + a, s_box[3u + a][s]); }
            s_key[s] = 0u; s_cnt[s] = 0u;
            for (uint32_t a = 0; a < 6u; a++) s_box[a][s] = a < 3u ? 0xffffffffu : 0u;
        }
        __syncthreads();
    }
}

template <int VOL>
__global__ __launch_bounds__(kLabelThreads) void label_mask_kernel(const VolumeDesc V, const LabelDesc D, const uint32_t *__restrict__ labels, const uint8_t *__restrict__ keep, void *__restrict__ out) {
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;
            if (i >= D.n) continue;
            uint32_t x, y, z;
            label_coords((uint32_t)i, D.nx, D.ny, x, y, z);
            const uint32_t m = keep[labels[i]];  // keep[0] == 0: background is never selected
            const uint32_t bits = (m != 0u) != (D.invert != 0u) ? voxel_texel_bits<VOL>(V, x, y, z) : D.fill_bits;
            store_texel_bits<texel_class(VOL)>(out, i, bits);
        }
    }
}

// ---- the kernels as another pass launches them (vk_label_launch.hpp) ----------------------------------------------------------------
void label_launch_tile(hipStream_t stream, uint32_t blocks, int kind, const VolumeDesc &V, const LabelDesc &D, uint32_t *parent) {
    with_scalar_kind(kind, [&](auto VOL) { hipLaunchKernelGGL(label_tile_kernel<VOL()>, dim3(blocks), dim3(kLabelThreads), 0, stream, V, D, parent); });
}
void label_launch_tile_words(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const LabelWords &W, uint32_t *parent) {
    hipLaunchKernelGGL(label_tile_words_kernel, dim3(blocks), dim3(kLabelThreads), 0, stream, W, D, parent);
}
void label_launch_seam(hipStream_t stream, uint32_t blocks, const LabelDesc &D, uint32_t *parent) {
    hipLaunchKernelGGL(label_seam_kernel, dim3(blocks), dim3(kLabelThreads), 0, stream, D, parent);
}
void label_launch_flatten(hipStream_t stream, uint32_t blocks, const LabelDesc &D, uint32_t *parent, uint32_t *chunk_roots, uint32_t *chunk_fg) {
    hipLaunchKernelGGL(label_flatten_kernel, dim3(blocks), dim3(kLabelThreads), 0, stream, D, parent, chunk_roots, chunk_fg);
}
void label_launch_scan(hipStream_t stream, uint32_t chunks, uint32_t *chunk_roots, const uint32_t *chunk_fg, unsigned long long *totals) {
    hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kLabelThreads), 0, stream, chunks, chunk_roots, chunk_fg, totals);
}
void label_launch_number(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const uint32_t *parent, const uint32_t *chunk_offset, uint32_t *labels, const LabelRecords &R) {
    hipLaunchKernelGGL(label_number_kernel, dim3(blocks), dim3(kLabelThreads), 0, stream, D, parent, chunk_offset, labels, R);
}
void label_launch_stats(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const uint32_t *parent, uint32_t *labels, const LabelRecords &R) {
    hipLaunchKernelGGL(label_stats_kernel, dim3(blocks), dim3(kLabelThreads), 0, stream, D, parent, labels, R);
}

extern "C" {

int vk_label_components(vk_ctx *ctx, const vk_label_request *req, const vk_voxel_box *box, uint32_t *labels_out, vk_component *components, uint64_t cap_components, void *dense_out,
                        vk_label_result *result) {
    static const char *const entry = "vk_label_components";
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = label_validate(req, labels_out != nullptr, components != nullptr, cap_components, dense_out != nullptr, result != nullptr))
        return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + why);
    const bool install = (req->flags & VK_LABEL_INSTALL) != 0u;
    if (int rc = pass_install_refused(ctx, entry, "VK_LABEL_INSTALL", install)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, entry, "label")) return rc;
    if (!label_seeds_inside(req, ctx->nx, ctx->ny, ctx->nz)) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": a seed lies outside the volume");
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, entry, "VK_LABEL_CLIP_BOX", box, (req->flags & VK_LABEL_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, entry, "label")) return rc;
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    if (!label_volume_fits(ctx->nx, ctx->ny, ctx->nz)) return fail(ctx, VK_ERR_UNSUPPORTED, "label: a volume of more than 2^32 - 2 voxels (labels are 32-bit)");

    const int kind = ctx->vol_kind;
    const FilterGrid G = filter_grid(ctx->nx, ctx->ny, ctx->nz, kLabelTile, ctx->label_max_blocks);
    LabelDesc D{};
    D.nx = ctx->nx; D.ny = ctx->ny; D.nz = ctx->nz;
    D.conn_sum = label_conn_sum(req->connectivity);
    D.box = B;
    D.ntx = G.ntx; D.nty = G.nty; D.tiles = G.tiles;
    D.n = n;
    D.chunks = label_chunks(n);
    D.lo_k = label_scale_bound(req->lo, ctx->format);
    D.hi_k = label_scale_bound(req->hi, ctx->format);
    D.fill_bits = label_fill_bits(req->fill, ctx->format);
    D.invert = (req->flags & VK_LABEL_INVERT) ? 1u : 0u;
    const uint32_t chunk_blocks = label_blocks(D.chunks, ctx->label_max_blocks);

    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, entry};
    // (debug, vk_debug_set_param("label_timing", k): phase k alone between the context's timer events, read with vk_timer_elapsed_ms --
    //  1 tile, 2 seam, 3 flatten, 4 scan, 5 number, 6 label, 7 mask)
    const uint32_t timing = ctx->label_timing;

    DeviceTemp d_parent, d_labels, d_chunk_roots, d_chunk_fg, d_totals;
    if (int rc = call.alloc(d_parent, (size_t)n * 4u, "the parent array")) return rc;
    if (int rc = call.alloc(d_labels, (size_t)n * 4u, "the label array")) return rc;
    if (int rc = call.alloc(d_chunk_roots, (size_t)D.chunks * 4u, "the chunk counts")) return rc;
    if (int rc = call.alloc(d_chunk_fg, (size_t)D.chunks * 4u, "the chunk counts")) return rc;
    if (int rc = call.alloc(d_totals, 16u, "the totals")) return rc;
    uint32_t *parent = (uint32_t *)d_parent.p, *labels = (uint32_t *)d_labels.p, *chunk_roots = (uint32_t *)d_chunk_roots.p, *chunk_fg = (uint32_t *)d_chunk_fg.p;

    call.phase(timing == 1u, [&] { with_scalar_kind(kind, [&](auto VOL) { hipLaunchKernelGGL(label_tile_kernel<VOL()>, dim3(G.blocks), dim3(kLabelThreads), 0, ctx->stream, V, D, parent); }); });
    call.phase(timing == 2u, [&] { hipLaunchKernelGGL(label_seam_kernel, dim3(G.blocks), dim3(kLabelThreads), 0, ctx->stream, D, parent); });
    call.phase(timing == 3u, [&] { hipLaunchKernelGGL(label_flatten_kernel, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, D, parent, chunk_roots, chunk_fg); });
    call.phase(timing == 4u, [&] { hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(kLabelThreads), 0, ctx->stream, D.chunks, chunk_roots, chunk_fg, (unsigned long long *)d_totals.p); });
    unsigned long long totals[2] = {0ull, 0ull};
    call.download(totals, d_totals.p, sizeof totals);
    if (int rc = call.finish()) return rc;
    const uint64_t n_comp = totals[0], n_fg = totals[1];

    DeviceTemp d_first, d_size, d_box;
    if (int rc = call.alloc(d_first, (size_t)n_comp * 4u, "the component records")) return rc;
    if (int rc = call.alloc(d_size, (size_t)n_comp * 4u, "the component records")) return rc;
    if (int rc = call.alloc(d_box, (size_t)n_comp * 24u, "the component records")) return rc;
    const LabelRecords R{(uint32_t *)d_first.p, (uint32_t *)d_size.p, (uint32_t *)d_box.p};
    if (n_comp) call.phase(timing == 5u, [&] { hipLaunchKernelGGL(label_number_kernel, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, D, parent, chunk_roots, labels, R); });
    call.phase(timing == 6u, [&] { hipLaunchKernelGGL(label_stats_kernel, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, D, parent, labels, R); });

    // the selection: host arithmetic over the sizes; the seeds' labels are a sixteen-word download
    std::vector<uint32_t> sizes((size_t)n_comp);
    uint32_t seed_labels[VK_LABEL_MAX_SEEDS] = {};
    if (n_comp) call.download(sizes.data(), R.size, (size_t)n_comp * 4u);
    for (uint32_t s = 0; s < req->n_seeds; s++) call.download(seed_labels + s, labels + voxel_index(req->seeds[s][0], req->seeds[s][1], req->seeds[s][2], D.nx, D.ny), 4u);
    if (int rc = call.finish()) return rc;
    std::vector<uint8_t> keep;
    uint64_t kept_voxels = 0;
    const uint64_t kept_comps = label_select(*req, sizes.data(), n_comp, seed_labels, keep, &kept_voxels);

    const size_t dense_bytes = pass_dense_bytes(ctx->format, n);
    DeviceTemp d_keep, d_out;
    if (dense_out || install) {
        if (int rc = call.alloc(d_keep, keep.size(), "the keep bytes")) return rc;
        if (int rc = call.alloc(d_out, dense_bytes, "the output buffer")) return rc;
        call.e = hipMemcpyAsync(d_keep.p, keep.data(), keep.size(), hipMemcpyHostToDevice, ctx->stream);
        call.phase(timing == 7u, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(label_mask_kernel<VOL()>, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, V, D, labels, (const uint8_t *)d_keep.p, d_out.p);
            });
        });
        call.download(dense_out, d_out.p, dense_bytes);
    }
    call.download(labels_out, labels, (size_t)n * 4u);
    const uint64_t n_rec = components ? (n_comp < cap_components ? n_comp : cap_components) : 0u;
    if (int rc = label_download_components(call, R, sizes.data(), n_rec, components)) return rc;
    if (result) *result = vk_label_result{n_comp, n_fg, kept_comps, kept_voxels};
    return install ? call.install(d_out, D.nx, D.ny, D.nz, ctx->format, ctx->layout) : VK_OK;
}

}  // extern "C"
