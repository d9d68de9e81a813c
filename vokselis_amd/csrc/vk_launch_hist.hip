// vk_launch_hist.hip -- the volume histogram and region statistics (vk_volume_histogram, vk_histogram_window).  A kernel
// family of its own: a reduction over the stored texels of a voxel box, no ray and no plane.  The classification of a texel, the key of min
// and max and all launch arithmetic are vk_hist.hpp's, shared with the host fuzz.
//
// Reading.  Where a cell is, its load, its taps and the decode of a texel are vk_texel.hpp's; which texels a lane takes is this unit's.
// LINEAR: the box is a set of runs of contiguous voxels (full rows merge into planes, full planes into one run); a lane loads
// one aligned 16-byte chunk of a run and masks the elements before the run's first and behind its last voxel.  Cell layouts: only the
// cells whose low-corner voxel is even on all three axes are read -- one in eight, every tap of them a voxel of its own -- one cell per
// lane, a wave taking 8 bricks along x with the 8 even cells of each; taps outside the box are masked, which also drops the duplicate the
// clamp baked into the last cell of an odd dimension (its voxel index equals the dimension, and the box ends there at the latest).
//
// Counting.  A workgroup keeps bins + 3 u32 counters in LDS (the bins, then NaN, below, above) and merges them into the u64 device
// counters with 64-bit integer atomics at its end, and earlier after hist_flush_passes() passes of its loop.  Real volumes are mostly one
// value, where a plain LDS add per voxel serialises: a lane counts runs of equal slots among its own elements (one add per run), and
// when every element of the whole wave falls into one slot -- air -- one lane adds the wave's voxel count.  Integer adds commute: the counts
// do not depend on the launch.
//
// Statistics.  min and max as maxima of ~key and key (hist_key), per lane, then one integer atomic per workgroup; sum and sum_sq in f64
// per lane, reduced over the wave by a butterfly and over the workgroup's four waves in order, stored as the workgroup's partial, which
// the host sums in block order: no float atomics, the same bits from run to run.
//
// Plain C++; no inline assembly.
#include "vk_launch.hpp"
#include "vk_hist.hpp"
#include "vk_texel.hpp"

#include <vector>

using namespace vk;

struct HistDesc {
    float lo_k, hi_k, k1, k2;
    uint32_t bins, flush_passes;
    uint32_t x0, y0, z0, x1, y1, z1;  // the voxel box
    uint64_t items;                   // LINEAR: chunks (runs x cpr); cells: wave items (segments of 8 bricks along x, x brick rows, x brick planes)
    uint64_t off0, len, sa, sb, cpr, total_bytes;  // LINEAR: hist_runs(), chunks per run, bytes of the array
    uint32_t na, nb;
    uint32_t bx0, by0, bz0, nsx, nby, nbz;         // cells: first brick per axis (in bricks of even cells), segments along x, bricks along y and z
    unsigned long long *out;          // counts[bins], NaN, below, above, n_finite, (max ~key, max key), then two f64 per block
    uint32_t pad[2];
};
static_assert(sizeof(HistDesc) % 8 == 0 && pass_kernargs_fit<HistDesc>, "hist kernels: VolumeDesc + HistDesc");

constexpr uint32_t kLdsCounters = VK_HIST_MAX_BINS + kHistCats;

struct HistAcc {
    double sum = 0.0, sq = 0.0;
    unsigned long long n_finite = 0;
    uint32_t inv_min = 0, max_key = 0;
    uint32_t vmin = 0xffffffffu, vmax = 0u;  // integer formats: min and max as integers, keyed once at the end (hist_acc_close)
};

// How a kernel's elements are counted, by the texel class of its kind (vk_common.hpp).  TEXEL_F16: e[] holds f32 bits, classified by
// hist_bin, keyed and summed in f64 one by one.  TEXEL_U16: e[] holds the integer value -- min and max as integers, the pass's sum and sum
// of squares as integers (8 x 65535^2 fits a u64), added to the f64 sums once per pass: the same sums, every partial an integer.
// TEXEL_U8: as TEXEL_U16, and the slot of each of the 256 values is read from a table the workgroup builds in LDS with hist_bin at its
// start (8 x 255^2 fits a u32).

__device__ __forceinline__ void hist_lds_clear(uint32_t *lds, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += kHistThreads) lds[i] = 0u;
    __syncthreads();
}
// the workgroup's counters into the device's, and back to zero
__device__ __forceinline__ void hist_lds_merge(uint32_t *lds, uint32_t n, unsigned long long *out) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += kHistThreads) {
        const uint32_t v = lds[i];
        if (v) { atomicAdd(out + i, (unsigned long long)v); lds[i] = 0u; }
    }
    __syncthreads();
}

// N elements of a lane (valid: bit e set where element e is a voxel of the box; the others hold 0) into the statistics and the workgroup's
// counters.  Called by whole waves: every lane of the wave is here, lanes without work with valid == 0.
template <int N, int FMT>
__device__ __forceinline__ void hist_count(uint32_t *lds, const uint16_t *lut, const HistDesc &D, const uint32_t (&el)[N], const uint32_t valid, HistAcc &A) {
    uint32_t slot[N];
    uint32_t s0 = 0u;
    bool have = false, same = true;
    uint32_t isum = 0u, isq32 = 0u;
    unsigned long long isq64 = 0ull;
#pragma unroll
    for (int e = 0; e < N; e++) {
        const bool v = (valid >> e) & 1u;
        if constexpr (FMT == TEXEL_F16) {
            const float x = __uint_as_float(el[e]);
            slot[e] = hist_slot(hist_bin(x, D.lo_k, D.hi_k, D.k1, D.k2, D.bins), D.bins);
            if (v) {
                if (x == x) {
                    const uint32_t k = hist_key(x);
                    A.inv_min = max(A.inv_min, ~k);
                    A.max_key = max(A.max_key, k);
                }
                if (fabsf(x) < __builtin_inff()) {
                    const double d = (double)x;
                    A.n_finite++;
                    A.sum += d;
                    A.sq = __builtin_fma(d, d, A.sq);
                }
            }
        } else {
            const uint32_t u = el[e];  // 0 where not valid: adds nothing to the sums and leaves vmax alone
            if constexpr (FMT == TEXEL_U8) slot[e] = lut[u & 0xffu];
            else slot[e] = hist_slot(hist_bin((float)u, D.lo_k, D.hi_k, D.k1, D.k2, D.bins), D.bins);
            A.vmin = min(A.vmin, v ? u : 0xffffffffu);
            A.vmax = max(A.vmax, u);
            isum += u;
            if constexpr (FMT == TEXEL_U8) isq32 += u * u;
            else isq64 += (unsigned long long)(u * u);  // u <= 65535: the product fits 32 bits
        }
        if (v) {
            if (!have) { s0 = slot[e]; have = true; }
            else same = same && slot[e] == s0;
        }
    }
    if constexpr (FMT != TEXEL_F16) {
        A.n_finite += (unsigned long long)__popc(valid);
        A.sum += (double)isum;
        A.sq += FMT == TEXEL_U8 ? (double)isq32 : (double)isq64;
    }
    const unsigned long long with_work = __ballot(have);
    if (with_work == 0ull) return;  // wave-uniform
    const uint32_t src = (uint32_t)__ffsll(with_work) - 1u;
    const uint32_t sf = (uint32_t)__builtin_amdgcn_readlane((int)s0, (int)src);
    if (__all(!have || (same && s0 == sf))) {
        // the whole wave in one slot: one add of its voxel count
        const uint32_t nv = (uint32_t)__popc(valid);
        uint32_t total;
        if (__all(!have || nv == (uint32_t)N)) total = (uint32_t)N * (uint32_t)__popcll(with_work);
        else {
            total = nv;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) total += (uint32_t)__shfl_xor((int)total, m);
        }
        if ((threadIdx.x & 63u) == src) atomicAdd(&lds[sf], total);
        return;
    }
    // runs of equal slots among the lane's elements: one add per run
    uint32_t cur = 0u, run = 0u;
#pragma unroll
    for (int e = 0; e < N; e++) {
        if ((valid >> e) & 1u) {
            if (run != 0u && slot[e] != cur) { atomicAdd(&lds[cur], run); run = 0u; }
            cur = slot[e];
            run++;
        }
    }
    if (run != 0u) atomicAdd(&lds[cur], run);
}

// the integer formats' min and max into the keys (a lane that saw no voxel keeps the empty marks)
template <int FMT>
__device__ __forceinline__ void hist_acc_close(HistAcc &A) {
    if constexpr (FMT != TEXEL_F16) {
        if (A.n_finite) { A.inv_min = ~hist_key((float)A.vmin); A.max_key = hist_key((float)A.vmax); }
    }
}

// the slots of the 256 values of a u8 format (kHistThreads == 256: one each)
template <int FMT>
__device__ __forceinline__ void hist_lut_build(uint16_t *lut, const HistDesc &D) {
    if constexpr (FMT == TEXEL_U8) lut[threadIdx.x] = (uint16_t)hist_slot(hist_bin((float)threadIdx.x, D.lo_k, D.hi_k, D.k1, D.k2, D.bins), D.bins);
}
static_assert(kHistThreads == 256u && VK_HIST_MAX_BINS + kHistCats <= 65535u, "the u8 table: one thread per value, a slot fits 16 bits");

// The lanes' statistics into the workgroup's partial (block order on the host), n_finite and the two keys.
__device__ __forceinline__ void hist_finish(HistAcc A, const HistDesc &D) {
    __shared__ double w_sum[4], w_sq[4];
    __shared__ unsigned long long w_fin[4];
    __shared__ uint32_t w_inv[4], w_max[4];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        A.sum += __shfl_xor(A.sum, m);
        A.sq += __shfl_xor(A.sq, m);
        A.n_finite += (unsigned long long)__shfl_xor((long long)A.n_finite, m);
        A.inv_min = max(A.inv_min, (uint32_t)__shfl_xor((int)A.inv_min, m));
        A.max_key = max(A.max_key, (uint32_t)__shfl_xor((int)A.max_key, m));
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) { w_sum[wave] = A.sum; w_sq[wave] = A.sq; w_fin[wave] = A.n_finite; w_inv[wave] = A.inv_min; w_max[wave] = A.max_key; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        double s = w_sum[0], q = w_sq[0];
        unsigned long long f = w_fin[0];
        uint32_t im = w_inv[0], mk = w_max[0];
        for (int w = 1; w < 4; w++) { s += w_sum[w]; q += w_sq[w]; f += w_fin[w]; im = max(im, w_inv[w]); mk = max(mk, w_max[w]); }
        unsigned long long *stat = D.out + D.bins + kHistCats;
        if (f) atomicAdd(stat, f);
        uint32_t *keys = reinterpret_cast<uint32_t *>(stat + 1);
        if (im) atomicMax(keys, im);
        if (mk) atomicMax(keys + 1, mk);
        double *part = reinterpret_cast<double *>(stat + 2) + 2u * (size_t)blockIdx.x;
        part[0] = s;
        part[1] = q;
    }
}

// a stored texel as hist_count's element: the f32 bits of a half, or the integer
template <int VOL>
__device__ __forceinline__ uint32_t hist_element(uint32_t bits) {
    if constexpr (texel_class(VOL) == TEXEL_F16) return __float_as_uint(texel_f32<VOL>(bits));
    else return bits;
}

// LINEAR: one aligned 16-byte chunk of a run per lane.
template <int VOL>
__global__ __launch_bounds__(kHistThreads) void hist_linear_kernel(const void *__restrict__ data, const HistDesc D) {
    __shared__ uint32_t lds[kLdsCounters];
    __shared__ uint16_t lut[256];
    constexpr uint32_t E = VOL == VOL_LINEAR_U8 ? 1u : 2u;
    constexpr int N = (int)(kHistLinearChunk / E);
    constexpr int FMT = texel_class(VOL);
    const uint32_t n_lds = D.bins + kHistCats;
    hist_lut_build<FMT>(lut, D);
    hist_lds_clear(lds, n_lds);
    const unsigned char *base = reinterpret_cast<const unsigned char *>(data);
    const bool one_run = D.na == 1u && D.nb == 1u;
    HistAcc A;
    uint32_t passes = 0u;
    for (uint64_t first = (uint64_t)blockIdx.x * kHistThreads; first < D.items; first += (uint64_t)gridDim.x * kHistThreads) {  // block-uniform
        const uint64_t item = first + threadIdx.x;
        uint32_t t[N];
#pragma unroll
        for (int e = 0; e < N; e++) t[e] = 0u;
        uint32_t valid = 0u;
        if (item < D.items) {
            uint64_t run = 0u, j = item;
            if (!one_run) { run = item / D.cpr; j = item - run * D.cpr; }
            const uint64_t b = run / D.na, a = run - b * D.na;
            const uint64_t s = D.off0 + a * D.sa + b * D.sb;              // the run's first voxel
            const uint64_t byte0 = s * E, byte1 = (s + D.len) * E;       // byte1 <= total_bytes: the box lies within the volume
            const uint64_t cb = ((byte0 >> 4) + j) << 4;                 // the chunk's first byte
            if (cb < byte1) {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (cb + kHistLinearChunk <= D.total_bytes) {
                    const uint4 q = *reinterpret_cast<const uint4 *>(base + cb);
                    w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
                } else {  // the array's last, partial chunk: byte by byte, nothing behind the array is read
#pragma unroll
                    for (uint32_t k = 0; k < kHistLinearChunk; k++)
                        if (cb + k < D.total_bytes) w[k >> 2] |= (uint32_t)base[cb + k] << (8u * (k & 3u));
                }
                const uint32_t e0 = cb >= byte0 ? 0u : (uint32_t)(byte0 - cb) / E;
                const uint32_t e1 = byte1 - cb >= kHistLinearChunk ? (uint32_t)N : (uint32_t)(byte1 - cb) / E;
                valid = ((1u << e1) - 1u) & ~((1u << e0) - 1u);
#pragma unroll
                for (int e = 0; e < N; e++) {  // (an element outside the run is 0: hist_count)
                    const uint32_t bits = texel_field<8 * (int)E>(w, (uint32_t)e);
                    t[e] = ((valid >> e) & 1u) ? hist_element<VOL>(bits) : 0u;
                }
            }
        }
        hist_count<N, FMT>(lds, lut, D, t, valid, A);
        if (++passes == D.flush_passes) { hist_lds_merge(lds, n_lds, D.out); passes = 0u; }
    }
    hist_lds_merge(lds, n_lds, D.out);
    hist_acc_close<FMT>(A);
    hist_finish(A, D);
}

// Cell layouts: the even cells, one per lane; a wave takes 8 bricks along x.
template <int VOL>
__global__ __launch_bounds__(kHistThreads) void hist_cells_kernel(const VolumeDesc V, const HistDesc D) {
    __shared__ uint32_t lds[kLdsCounters];
    __shared__ uint16_t lut[256];
    constexpr int FMT = texel_class(VOL);
    const uint32_t n_lds = D.bins + kHistCats;
    hist_lut_build<FMT>(lut, D);
    hist_lds_clear(lds, n_lds);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    HistAcc A;
    uint32_t passes = 0u;
    for (uint64_t first = (uint64_t)blockIdx.x * 4u; first < D.items; first += (uint64_t)gridDim.x * 4u) {  // block-uniform
        const uint64_t w = first + wave;  // wave-uniform
        uint32_t t[8];
#pragma unroll
        for (int b = 0; b < 8; b++) t[b] = 0u;
        uint32_t valid = 0u;
        if (w < D.items) {
            const uint64_t rest = w / D.nsx;
            const uint32_t seg = (uint32_t)(w - rest * D.nsx);
            const uint32_t bz = (uint32_t)(rest / D.nby), by = (uint32_t)(rest - (uint64_t)bz * D.nby);
            // the lane's even cell: brick (bx0 + 8 seg + lane / 8, by0 + by, bz0 + bz), the brick's even cell (lane & 7); its low-corner voxel
            const uint32_t ix = 4u * (D.bx0 + seg * 8u + (lane >> 3)) + 2u * (lane & 1u);
            const uint32_t iy = 4u * (D.by0 + by) + 2u * ((lane >> 1) & 1u);
            const uint32_t iz = 4u * (D.bz0 + bz) + 2u * ((lane >> 2) & 1u);
            const uint32_t vx = (ix >= D.x0 && ix < D.x1 ? 1u : 0u) | (ix + 1u >= D.x0 && ix + 1u < D.x1 ? 2u : 0u);
            const uint32_t vy = (iy >= D.y0 && iy < D.y1 ? 1u : 0u) | (iy + 1u >= D.y0 && iy + 1u < D.y1 ? 2u : 0u);
            const uint32_t vz = (iz >= D.z0 && iz < D.z1 ? 1u : 0u) | (iz + 1u >= D.z0 && iz + 1u < D.z1 ? 2u : 0u);
#pragma unroll
            for (int b = 0; b < 8; b++)
                if (((vx >> (b & 1)) & 1u) && ((vy >> ((b >> 1) & 1)) & 1u) && ((vz >> (b >> 2)) & 1u)) valid |= 1u << b;
            if (valid) {  // a tap inside the box: ix, iy, iz lie inside the volume, the cell exists
                uint32_t c[cell_words(VOL)];
                load_cell<VOL>(cell_ptr(V, ix, iy, iz), c);
#pragma unroll
                for (int b = 0; b < 8; b++) t[b] = hist_element<VOL>(cell_tap_bits<VOL>(c, (uint32_t)b));
#pragma unroll
                for (int b = 0; b < 8; b++)
                    if (!((valid >> b) & 1u)) t[b] = 0u;  // (an element outside the box is 0: hist_count)
            }
        }
        hist_count<8, FMT>(lds, lut, D, t, valid, A);
        if (++passes == D.flush_passes) { hist_lds_merge(lds, n_lds, D.out); passes = 0u; }
    }
    hist_lds_merge(lds, n_lds, D.out);
    hist_acc_close<FMT>(A);
    hist_finish(A, D);
}

int vk_volume_histogram(vk_ctx *ctx, const vk_histogram *hist, const vk_voxel_box *box, uint64_t *counts, vk_volume_stats *stats) {
    if (!ctx) return VK_ERR_INVALID;
    HistConsts K{};
    if (const char *why = hist_validate(hist, format_scale(ctx->format), K)) return fail(ctx, VK_ERR_INVALID, std::string("vk_volume_histogram: ") + why);
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, "vk_volume_histogram", "histogram")) return rc;
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, "vk_volume_histogram", "VK_HIST_CLIP_BOX", box, (hist->flags & VK_HIST_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, "vk_volume_histogram", "histogram")) return rc;
    const uint64_t n_voxels = voxel_box_voxels(B);

    const int kind = ctx->vol_kind;
    const bool cells = is_cell_layout(kind);
    HistDesc D{};
    D.lo_k = K.lo_k; D.hi_k = K.hi_k; D.k1 = K.k1; D.k2 = K.k2; D.bins = K.bins;
    D.x0 = B.x0; D.y0 = B.y0; D.z0 = B.z0; D.x1 = B.x1; D.y1 = B.y1; D.z1 = B.z1;
    uint32_t per_block, pass_voxels;
    if (cells) {
        uint32_t nbx;
        hist_cell_range(B.x0, B.x1, D.bx0, nbx);
        hist_cell_range(B.y0, B.y1, D.by0, D.nby);
        hist_cell_range(B.z0, B.z1, D.bz0, D.nbz);
        D.nsx = (nbx + 7u) / 8u;
        D.items = (uint64_t)D.nsx * D.nby * D.nbz;
        per_block = kHistThreads / 64u;
        pass_voxels = hist_pass_voxels_cells();
    } else {
        const uint32_t elem = kind == VOL_LINEAR_U8 ? 1u : 2u;
        const HistRuns R = hist_runs(B, ctx->nx, ctx->ny);
        D.off0 = R.off0; D.len = R.len; D.sa = R.sa; D.sb = R.sb; D.na = R.na ? R.na : 1u; D.nb = R.nb ? R.nb : 1u;
        D.cpr = hist_run_chunks(R.len, elem);
        D.items = n_voxels ? D.cpr * R.na * R.nb : 0u;
        D.total_bytes = (uint64_t)ctx->nx * ctx->ny * ctx->nz * elem;
        per_block = kHistThreads;
        pass_voxels = hist_pass_voxels_linear(elem);
    }
    if (n_voxels == 0u) D.items = 0u;
    D.flush_passes = ctx->hist_flush_passes ? ctx->hist_flush_passes : hist_flush_passes(pass_voxels);
    const uint32_t grid = hist_grid(D.items, per_block, (uint32_t)ctx->prop.multiProcessorCount, ctx->hist_max_blocks);

    const size_t words = (size_t)K.bins + kHistCats + 2u + 2u * (size_t)grid;
    std::vector<unsigned long long> h(words, 0ull);
    if (D.items) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        DeviceTemp d;
        PassCall call{ctx, "vk_volume_histogram"};
        if (int rc = call.alloc(d, words * sizeof(unsigned long long), "the counters")) return rc;
        D.out = reinterpret_cast<unsigned long long *>(d.p);
        call.e = hipMemsetAsync(d.p, 0, words * sizeof(unsigned long long), ctx->stream);
        call.phase(false, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                if constexpr (is_cell_layout(VOL())) hipLaunchKernelGGL(hist_cells_kernel<VOL()>, dim3(grid), dim3(kHistThreads), 0, ctx->stream, volume_desc(ctx), D);
                else hipLaunchKernelGGL(hist_linear_kernel<VOL()>, dim3(grid), dim3(kHistThreads), 0, ctx->stream, (const void *)ctx->vol, D);
            });
        });
        call.download(h.data(), d.p, words * sizeof(unsigned long long));
        if (int rc = call.finish()) return rc;
    }
    if (counts)
        for (uint32_t i = 0; i < K.bins; i++) counts[i] = h[i];
    if (stats) {
        vk_volume_stats s{};
        s.n_voxels = n_voxels;
        s.n_nan = h[K.bins]; s.n_below = h[K.bins + 1u]; s.n_above = h[K.bins + 2u];
        s.n_finite = h[K.bins + kHistCats];
        uint32_t keys[2];
        memcpy(keys, &h[K.bins + kHistCats + 1u], sizeof(keys));
        hist_minmax_decode(keys[0], keys[1], s.min, s.max);
        for (uint32_t b = 0; b < grid; b++) {  // block order
            double part[2];
            memcpy(part, &h[K.bins + kHistCats + 2u + 2u * (size_t)b], sizeof(part));
            s.sum += part[0];
            s.sum_sq += part[1];
        }
        s.scale = (float)sample_scale(format_scale(ctx->format));
        *stats = s;
    }
    return VK_OK;
}

int vk_histogram_window(const uint64_t *counts, uint32_t bins, float lo, float hi, double p_lo, double p_hi, float *w_lo, float *w_hi) {
    if (!w_lo || !w_hi) return fail(nullptr, VK_ERR_INVALID, "vk_histogram_window: NULL argument");
    float a, b;
    if (const char *why = hist_window(counts, bins, lo, hi, p_lo, p_hi, a, b)) return fail(nullptr, VK_ERR_INVALID, std::string("vk_histogram_window: ") + why);
    *w_lo = a;
    *w_hi = b;
    return VK_OK;
}
