// vk_launch_measure.hip -- measure labelled regions (vk_measure_components): the volume and a label array are
// reduced into one exact integer record per region.  The request's validation, q, the limbs, the closed forms of a run and the record's
// layout are vk_measure.hpp's, shared with the host fuzz.  The label pass's tile / seam / flatten / scan / number / stats kernels
// (vk_label_launch.hpp) are borrowed as they are where the caller brings no labels; the kernels here are the maximum, the records' initial
// values and the measure kernel.
//
//   labels   without labels_in: tile, seam, flatten, scan, number, stats -- the label array of vk_label_components, left on the device.
//            with labels_in: the upload, then the largest id and the labelled voxels in one pass (the host refuses an id above max_label).
//   init     every word of every record takes its operation's neutral element.
//   measure  one kernel per volume kind, in the chunked raster order of label_stats_kernel: a wave holds 64 consecutive voxels, a run is a
//            stretch of consecutive lanes with one id in one row.  A voxel's own terms -- q's limbs, its extremes, the exposed faces -- are
//            summed along the run by a segmented shuffle reduction (six steps, each bounded by the run's end); the run's head lane adds the
//            closed forms of the index sums and sends everything to the workgroup's table in LDS, or to memory where the slot is taken.
// Segmented reduction or a head lane walking its run's lanes: the reduction costs 6 steps x (13 dword shuffles for R16F, 6 for the integer
// formats) per wave whatever the runs are; the walk costs the same shuffles per LANE of the longest run with every other lane idle,
// 64 x 13 for a wave inside one grain -- the common case.  The reduction it is.
// The table: a record is 28 words of 64 bits (24 for the integer formats, whose kernels never touch the last four), so label_stats_kernel's
// 512 slots would need 112 KiB.  128 slots are 28 KiB (24 KiB): five (six) workgroups of 256 threads fit the CU's 160 KiB, 20 (24) waves
// per CU, which is what the kernel's registers allow anyway; 256 slots would leave two workgroups, 8 waves, too few to hide the label and
// texel loads.  A chunk of 4096 voxels of a grain scan holds a handful of ids; an id whose slot is taken goes to memory directly.
// Phases are separated by kernel boundaries: no flags, tickets or grid barriers, no float atomics, and no kernel here reads an address
// that another thread of the same launch writes.  Every sum is of integers and min / max commute: the records are the same bits for every
// launch shape.  Plain C++; no inline assembly.  wave64 is assumed in measure_kernel (the ballot is 64 bits wide).
#include "vk_label_launch.hpp"
#include "vk_measure.hpp"
#include "vk_pass_blocks.hpp"
#include "vk_texel.hpp"

#include <vector>

using namespace vk;

typedef unsigned long long measure_word;  // the device's 64-bit atomics are declared on this type
static_assert(sizeof(measure_word) == 8 && kMeasureSlots * 2u == kLabelThreads, "the flush: two threads per slot");

// the largest id and the labelled voxels: totals = {max, foreground}, zeroed before
__global__ __launch_bounds__(kLabelThreads) void measure_max_kernel(const LabelDesc D, const uint32_t *__restrict__ labels, measure_word *totals) {
    __shared__ measure_word s_max, s_fg;
    if (threadIdx.x == 0) { s_max = 0ull; s_fg = 0ull; }
    __syncthreads();
    uint32_t most = 0u, fg = 0u;
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;
            if (i >= D.n) continue;
            const uint32_t id = labels[i];
            most = id > most ? id : most;
            fg += id != 0u;
        }
    }
    if (most) __hip_atomic_fetch_max(&s_max, (measure_word)most, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    block_add(&s_fg, fg);
    __syncthreads();
    if (threadIdx.x == 0 && s_fg) {
        __hip_atomic_fetch_max(totals, s_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(totals + 1, s_fg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kLabelThreads) void measure_init_kernel(uint64_t words, measure_word *__restrict__ rec) {
    for (uint64_t e = (uint64_t)blockIdx.x * kLabelThreads + threadIdx.x; e < words; e += (uint64_t)gridDim.x * kLabelThreads) rec[e] = measure_word_init((uint32_t)(e % kMeasureWords));
}

// one word of a record takes v by the word's operation; SCOPE: the workgroup's table in LDS, or memory
template <int SCOPE>
__device__ __forceinline__ void measure_gather(measure_word *p, uint32_t k, uint64_t v) {
    switch (measure_word_op(k)) {
        case MOP_UMIN: __hip_atomic_fetch_min(p, (measure_word)v, __ATOMIC_RELAXED, SCOPE); break;
        case MOP_UMAX: __hip_atomic_fetch_max(p, (measure_word)v, __ATOMIC_RELAXED, SCOPE); break;
        case MOP_SMIN: __hip_atomic_fetch_min(reinterpret_cast<long long *>(p), (long long)v, __ATOMIC_RELAXED, SCOPE); break;
        case MOP_SMAX: __hip_atomic_fetch_max(reinterpret_cast<long long *>(p), (long long)v, __ATOMIC_RELAXED, SCOPE); break;
        default: __hip_atomic_fetch_add(p, (measure_word)v, __ATOMIC_RELAXED, SCOPE); break;
    }
}

// where a run's terms go: word k of the slot's column in LDS, or of the region's record in memory
struct MeasureLdsSink {
    measure_word *col;  // &table[0][slot]
    __device__ __forceinline__ void operator()(uint32_t k, uint64_t v) const { measure_gather<__HIP_MEMORY_SCOPE_WORKGROUP>(col + (size_t)k * kMeasureSlots, k, v); }
};
struct MeasureMemorySink {
    measure_word *rec;
    __device__ __forceinline__ void operator()(uint32_t k, uint64_t v) const { measure_gather<__HIP_MEMORY_SCOPE_AGENT>(rec + k, k, v); }
};

// v summed (OP) over the lanes lane .. end - 1 of the wave, for every lane at once: after step d a lane holds its next 2 d lanes' terms
// as far as they lie before `end`, the end of the lane's run.  Every lane of the wave takes part in every shuffle.
template <class T, class OP>
__device__ __forceinline__ T measure_run_reduce(T v, uint32_t lane, uint32_t end, OP op) {
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const T t = __shfl_down(v, d);
        if (lane + d < end) v = op(v, t);
    }
    return v;
}

// what a run's head lane holds after the reductions
struct MeasureRun {
    uint32_t counts;          // nonfinite voxels in bits 0 .. 7, exposed faces across x, y, z in bits 8 .. 15, 16 .. 23, 24 .. 31 (at most 128 each)
    int64_t q_min, q_max;
    int64_t q_hi;             // R16F alone
    uint64_t q_lo, qq[3];     // the integer formats: q and q q whole in q_lo and qq[0]
};

template <bool F16, class SINK>
__device__ __forceinline__ void measure_deposit(const SINK &sink, uint64_t i, uint32_t x, uint32_t y, uint32_t z, uint32_t len, const MeasureRun &r) {
    sink(MW_N, len);
    sink(MW_FIRST, i);
    sink(MW_BOX_LO, x); sink(MW_BOX_LO + 1u, y); sink(MW_BOX_LO + 2u, z);
    sink(MW_BOX_HI, x + len - 1u); sink(MW_BOX_HI + 1u, y); sink(MW_BOX_HI + 2u, z);
    uint64_t s[9];
    measure_run_sums(x, y, z, len, s);
#pragma unroll
    for (uint32_t k = 0; k < 9u; k++)
        if (s[k]) sink(MW_SUMS + k, s[k]);
#pragma unroll
    for (uint32_t a = 0; a < 3u; a++) {
        const uint32_t f = (r.counts >> (8u + 8u * a)) & 0xffu;
        if (f) sink(MW_FACES + a, f);
    }
    const uint32_t nonfinite = r.counts & 0xffu;
    if (nonfinite < len) {  // a finite voxel
        sink(MW_QMIN, (uint64_t)r.q_min);
        sink(MW_QMAX, (uint64_t)r.q_max);
        if (r.q_lo) sink(MW_Q_LO, r.q_lo);
        if (r.qq[0]) sink(MW_QQ0, r.qq[0]);
        if constexpr (F16) {
            if (r.q_hi) sink(MW_Q_HI, (uint64_t)r.q_hi);
            if (r.qq[1]) sink(MW_QQ1, r.qq[1]);
            if (r.qq[2]) sink(MW_QQ2, r.qq[2]);
        }
    }
    if constexpr (F16)
        if (nonfinite) sink(MW_NONFINITE, nonfinite);
}

// labels: 0 background, 1 .. n_regions; rec: kMeasureWords words per region, initialised.  The table's scheme is label_stats_kernel's:
// the first id to ask owns a slot until the chunk ends, an id that finds its slot taken goes to memory, and after the chunk two threads
// per used slot send the sums on.
template <int VOL>
__global__ __launch_bounds__(kLabelThreads) void measure_kernel(const VolumeDesc V, const LabelDesc D, const uint32_t *__restrict__ labels, uint32_t n_regions, measure_word *rec) {
    constexpr bool F16 = is_f16_kind(VOL);
    constexpr uint32_t W = F16 ? kMeasureWords : kMeasureWordsInt;
    static_assert(W % 2u == 0u, "the flush: a thread takes half a slot's words");
    __shared__ uint32_t s_key[kMeasureSlots];
    __shared__ measure_word s_tab[W][kMeasureSlots];
    for (uint32_t e = threadIdx.x; e < W * kMeasureSlots; e += kLabelThreads) s_tab[e / kMeasureSlots][e % kMeasureSlots] = measure_word_init(e / kMeasureSlots);
    if (threadIdx.x < kMeasureSlots) s_key[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t row = D.nx, slice = (uint64_t)D.nx * D.ny;
    for (uint32_t chunk = blockIdx.x; chunk < D.chunks; chunk += gridDim.x) {  // block-uniform
        for (uint32_t k = 0; k < kLabelChunkPerThread; k++) {
            const uint64_t i = (uint64_t)chunk * kLabelChunk + k * kLabelThreads + threadIdx.x;  // a wave: 64 consecutive voxels
            uint32_t id = 0u, x = 0u, y = 0u, z = 0u;
            if (i < D.n) {
                id = labels[i];
                if (id > n_regions) id = 0u;  // (the host has refused such an array: no record lies behind the last)
                label_coords((uint32_t)i, D.nx, D.ny, x, y, z);
            }
            const uint32_t prev = (uint32_t)__shfl_up((int)id, 1), next = (uint32_t)__shfl_down((int)id, 1);
            const bool boundary = lane == 0u || prev != id || x == 0u;  // a run starts here (of a region, or of background)
            const unsigned long long starts = __ballot(boundary);
            const unsigned long long after = lane == 63u ? 0ull : starts >> (lane + 1u);
            const uint32_t to_end = after ? (uint32_t)__ffsll(after) : 64u - lane;  // to the next start, or to the wave's end
            const uint32_t end = lane + to_end;

            // this voxel's own terms; a background voxel loads nothing and adds nothing
            MeasureRun t{};
            t.q_min = INT64_MAX; t.q_max = INT64_MIN;
            if (id != 0u) {
                const uint32_t bits = voxel_texel_bits<VOL>(V, x, y, z);
                bool finite = true;
                int64_t q;
                if constexpr (F16) q = measure_q_half(bits, finite); else q = (int64_t)bits;
                if (finite) {
                    t.q_min = t.q_max = q;
                    if constexpr (F16) { measure_q_split(q, t.q_hi, t.q_lo); measure_qq_split(q, t.qq); }
                    else { t.q_lo = (uint64_t)q; t.qq[0] = (uint64_t)q * (uint64_t)q; }
                }
                // the six neighbours' labels: across x from the lanes beside this one, with a load at the wave's ends; a neighbour outside the volume is 0
                const uint32_t xm = x == 0u ? 0u : (lane == 0u ? labels[i - 1u] : prev);
                const uint32_t xp = x + 1u == D.nx ? 0u : (lane == 63u ? labels[i + 1u] : next);
                const uint32_t ym = y == 0u ? 0u : labels[i - row], yp = y + 1u == D.ny ? 0u : labels[i + row];
                const uint32_t zm = z == 0u ? 0u : labels[i - slice], zp = z + 1u == D.nz ? 0u : labels[i + slice];
                t.counts = (finite ? 0u : 1u) | (((xm != id) + (xp != id)) << 8) | (((ym != id) + (yp != id)) << 16) | (((zm != id) + (zp != id)) << 24);
            }
            auto add = [](auto a, auto b) { return a + b; };
            t.counts = measure_run_reduce(t.counts, lane, end, add);
            if constexpr (F16) {
                t.q_min = measure_run_reduce((long long)t.q_min, lane, end, [](long long a, long long b) { return a < b ? a : b; });
                t.q_max = measure_run_reduce((long long)t.q_max, lane, end, [](long long a, long long b) { return a > b ? a : b; });
                t.q_hi = measure_run_reduce((int)t.q_hi, lane, end, add);            // |hi| <= 2^20, 64 of them
                t.q_lo = measure_run_reduce((uint32_t)t.q_lo, lane, end, add);       // < 2^20, 64 of them
#pragma unroll
                for (uint32_t m = 0; m < 3u; m++) t.qq[m] = measure_run_reduce((unsigned long long)t.qq[m], lane, end, add);  // < 2^28, 64 of them: 34 bits
            } else {
                // q < 2^16: the extremes travel as 32-bit words, INT64_MAX / INT64_MIN as 0xffffffff / 0
                const uint32_t lo = measure_run_reduce(t.q_min == INT64_MAX ? 0xffffffffu : (uint32_t)t.q_min, lane, end, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
                const uint32_t hi = measure_run_reduce(t.q_max == INT64_MIN ? 0u : (uint32_t)t.q_max, lane, end, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
                t.q_min = lo; t.q_max = hi;  // (a run of an integer format has no nonfinite voxel: both are values)
                t.q_lo = measure_run_reduce((uint32_t)t.q_lo, lane, end, add);       // < 2^16, 64 of them
                t.qq[0] = measure_run_reduce((unsigned long long)t.qq[0], lane, end, add);
            }

            if (id != 0u && boundary) {
                const uint32_t slot = measure_slot(id);
                const uint32_t owner = atomicCAS(&s_key[slot], 0u, id);
                if (owner == 0u || owner == id) measure_deposit<F16>(MeasureLdsSink{&s_tab[0][slot]}, i, x, y, z, to_end, t);
                else measure_deposit<F16>(MeasureMemorySink{rec + (size_t)(id - 1u) * kMeasureWords}, i, x, y, z, to_end, t);
            }
        }
        __syncthreads();
        {
            const uint32_t slot = threadIdx.x & (kMeasureSlots - 1u), half = threadIdx.x >> kMeasureSlotBits;
            const uint32_t id = s_key[slot];
            if (id != 0u) {
                measure_word *r = rec + (size_t)(id - 1u) * kMeasureWords;
#pragma unroll
                for (uint32_t w = 0; w < W; w++) {
                    if (w / (W / 2u) != half) continue;
                    const measure_word v = s_tab[w][slot];
                    if (v != measure_word_init(w)) measure_gather<__HIP_MEMORY_SCOPE_AGENT>(r + w, w, v);
                    s_tab[w][slot] = measure_word_init(w);
                }
            }
        }
        __syncthreads();  // both halves have read the key
        if (threadIdx.x < kMeasureSlots) s_key[threadIdx.x] = 0u;
        __syncthreads();
    }
}

extern "C" {

int vk_measure_components(vk_ctx *ctx, const vk_measure_request *req, const vk_voxel_box *box, const uint32_t *labels_in, vk_region *regions, uint64_t cap_regions,
                          vk_measure_result *result) {
    static const char *const entry = "vk_measure_components";
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = measure_validate(req, labels_in != nullptr, box != nullptr, regions != nullptr, cap_regions, result != nullptr))
        return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + why);
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, entry, "measure")) return rc;
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, entry, "VK_MEASURE_CLIP_BOX", box, (req->flags & VK_MEASURE_CLIP_BOX) != 0u, B)) return rc;
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    if (labels_in && req->max_label > n) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": max_label exceeds the voxel count");
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, entry, "measure")) return rc;
    if (!label_volume_fits(ctx->nx, ctx->ny, ctx->nz)) return fail(ctx, VK_ERR_UNSUPPORTED, "measure: a volume of more than 2^32 - 2 voxels (labels are 32-bit)");
    if (!measure_sums_fit(ctx->nx, ctx->ny, ctx->nz))
        return fail(ctx, VK_ERR_UNSUPPORTED, "measure: n (max dimension - 1)^2 exceeds 64 bits: a sum of index products could overflow");

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
    const uint32_t chunk_blocks = label_blocks(D.chunks, ctx->label_max_blocks);

    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, entry};
    // (debug, vk_debug_set_param("measure_timing", k): phase k alone between the context's timer events, read with vk_timer_elapsed_ms --
    //  1 tile and seam, 2 flatten and scan, 3 number and stats; with labels_in 1 the upload and the maximum; 4 init, 5 measure)
    const uint32_t timing = ctx->measure_timing;

    DeviceTemp d_parent, d_labels, d_chunk_roots, d_chunk_fg, d_totals, d_first, d_size, d_box;
    if (int rc = call.alloc(d_labels, (size_t)n * 4u, "the label array")) return rc;
    if (int rc = call.alloc(d_totals, 16u, "the totals")) return rc;
    uint32_t *labels = (uint32_t *)d_labels.p;
    unsigned long long totals[2] = {0ull, 0ull};
    uint64_t n_reg = 0, n_fg = 0;
    if (labels_in) {
        call.phase(timing == 1u, [&] {
            call.e = hipMemcpyAsync(labels, labels_in, (size_t)n * 4u, hipMemcpyHostToDevice, ctx->stream);
            if (call.e == hipSuccess) call.e = hipMemsetAsync(d_totals.p, 0, 16u, ctx->stream);
            if (call.e == hipSuccess) hipLaunchKernelGGL(measure_max_kernel, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, D, (const uint32_t *)labels, (measure_word *)d_totals.p);
        });
        call.download(totals, d_totals.p, sizeof totals);
        if (int rc = call.finish()) return rc;
        if (totals[0] > req->max_label) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": labels_in holds an id above max_label");
        n_reg = req->max_label;
        n_fg = totals[1];
    } else {
        if (int rc = call.alloc(d_parent, (size_t)n * 4u, "the parent array")) return rc;
        if (int rc = call.alloc(d_chunk_roots, (size_t)D.chunks * 4u, "the chunk counts")) return rc;
        if (int rc = call.alloc(d_chunk_fg, (size_t)D.chunks * 4u, "the chunk counts")) return rc;
        uint32_t *parent = (uint32_t *)d_parent.p, *chunk_roots = (uint32_t *)d_chunk_roots.p, *chunk_fg = (uint32_t *)d_chunk_fg.p;
        call.phase(timing == 1u, [&] {
            label_launch_tile(ctx->stream, G.blocks, kind, V, D, parent);
            label_launch_seam(ctx->stream, G.blocks, D, parent);
        });
        call.phase(timing == 2u, [&] {
            label_launch_flatten(ctx->stream, chunk_blocks, D, parent, chunk_roots, chunk_fg);
            label_launch_scan(ctx->stream, D.chunks, chunk_roots, chunk_fg, (unsigned long long *)d_totals.p);
        });
        call.download(totals, d_totals.p, sizeof totals);
        if (int rc = call.finish()) return rc;
        n_reg = totals[0];
        n_fg = totals[1];
        if (int rc = call.alloc(d_first, (size_t)n_reg * 4u, "the component records")) return rc;
        if (int rc = call.alloc(d_size, (size_t)n_reg * 4u, "the component records")) return rc;
        if (int rc = call.alloc(d_box, (size_t)n_reg * 24u, "the component records")) return rc;
        const LabelRecords R{(uint32_t *)d_first.p, (uint32_t *)d_size.p, (uint32_t *)d_box.p};
        call.phase(timing == 3u, [&] {
            if (n_reg) label_launch_number(ctx->stream, chunk_blocks, D, parent, chunk_roots, labels, R);
            label_launch_stats(ctx->stream, chunk_blocks, D, parent, labels, R);
        });
    }

    const uint64_t n_rec = regions ? (n_reg < cap_regions ? n_reg : cap_regions) : 0u;
    DeviceTemp d_rec;
    std::vector<uint64_t> words((size_t)n_rec * kMeasureWords);
    if (n_rec) {  // (the totals alone need no record)
        const uint64_t rec_words = n_reg * kMeasureWords;
        if (int rc = call.alloc(d_rec, (size_t)rec_words * 8u, "the region records")) return rc;
        measure_word *rec = (measure_word *)d_rec.p;
        call.phase(timing == 4u, [&] {
            hipLaunchKernelGGL(measure_init_kernel, dim3(label_blocks((rec_words + kLabelThreads - 1u) / kLabelThreads, ctx->label_max_blocks)), dim3(kLabelThreads), 0, ctx->stream, rec_words, rec);
        });
        call.phase(timing == 5u, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(measure_kernel<VOL()>, dim3(chunk_blocks), dim3(kLabelThreads), 0, ctx->stream, V, D, (const uint32_t *)labels, (uint32_t)n_reg, rec);
            });
        });
        call.download(words.data(), rec, words.size() * 8u);
    }
    if (int rc = call.finish()) return rc;
    for (uint64_t c = 0; c < n_rec; c++) regions[c] = measure_region(words.data() + c * kMeasureWords);
    if (result) *result = vk_measure_result{n_reg, n_fg, n_rec, measure_scale(ctx->format), 0u};
    return VK_OK;
}

}  // extern "C"
