// vk_launch_dist.hip -- exact Euclidean distance transform of a value range and morphology by a radius (vk_distance_transform; DESIGN.md
// section 25).  The request's validation, the overflow bound, what each round measures and the line function are vk_dist.hpp's, shared
// with the host fuzz; the predicate, its bounds and the fill rule are the label pass's (vk_label.hpp).
//
//   column   along z, one kernel per source of the predicate (a volume kind through vk_texel.hpp, or the first round's D2 against R2, read in
//            place).  A thread owns an (x, y) column, lanes along x: one sweep up leaves the steps to the nearest target below, one sweep
//            down takes the minimum with the steps to the nearest above and leaves (w steps)^2, or INF.
//   line y   a thread owns an (x, z) line, lanes along x: dist_line over entries nx apart, so the lanes' accesses are consecutive.
//   line x   every slice is transposed through LDS (x and y change places), the same kernel runs along what is now the strided axis, and
//            the result is transposed back: two passes at the speed of a copy buy the x pass the y pass's coalescing.  The plain form --
//            the line function along rows, lanes nx apart -- stays behind vk_debug_set_param("dist_x_plain", 1) for the comparison.
//   stats    (distance ops) zeros and the largest finite value, as one pair of partial results per workgroup.
//   mask     (morphology ops) one kernel per volume kind: S from the volume, M from the last D2, then the stored texel or a fill, and
//            four counts per workgroup.
// A round is column, line y, line x; CLOSE and OPEN run two, the second with the first's D2 as its predicate.  Phases are separated by
// kernel boundaries: no workgroup waits for another, and no address is written by two threads of a launch.  Integers only; plain C++,
// no inline assembly, no per-thread arrays.  Every loop has a bound: the grid-stride loops their item count, the sweeps nz, dist_line
// 2 n and n (vk_dist.hpp).  The counts reach memory as per-workgroup partial results that the host adds: no global atomics at all.
#include "vk_dist_launch.hpp"
#include "vk_label.hpp"
#include "vk_pass_blocks.hpp"
#include "vk_texel.hpp"

using namespace vk;

constexpr uint32_t kDistThreads = 256;

struct DistDesc {
    uint32_t nx, ny, nz, above;  // above: M = { D2 > R2 }, not { D2 <= R2 }
    uint64_t n, slice;           // voxels; nx ny
    uint64_t r2;
    uint32_t w[3], complement;   // complement: the first round measures to not S
    vk_voxel_box box;
    float lo_k, hi_k;
    uint32_t fill_in_bits, fill_out_bits;
};
static_assert(sizeof(DistDesc) % 8 == 0 && pass_kernargs_fit<DistDesc>, "distance kernels: VolumeDesc + DistDesc");

// the first round's target: S, or its complement
template <int VOL>
struct DistVolumeTarget {
    VolumeDesc V;
    __device__ __forceinline__ bool in_set(const DistDesc &D, uint32_t x, uint32_t y, uint32_t z) const {
        return label_in_box(x, y, z, D.box) && label_foreground(texel_f32<VOL>(voxel_texel_bits<VOL>(V, x, y, z)), D.lo_k, D.hi_k);
    }
    __device__ __forceinline__ bool operator()(const DistDesc &D, uint32_t x, uint32_t y, uint32_t z, uint64_t) const { return in_set(D, x, y, z) != (D.complement != 0u); }
};
// the second round's: the voxels whose first-round D2 lies above R2.  a is the array the column kernel writes: a thread reads an entry
// before it writes that same entry, and no other thread touches it.
struct DistAboveTarget {
    const uint32_t *a;
    __device__ __forceinline__ bool operator()(const DistDesc &D, uint32_t, uint32_t, uint32_t, uint64_t i) const { return (uint64_t)a[i] > D.r2; }
};

template <class T>
__global__ __launch_bounds__(kDistThreads) void dist_column_kernel(const T target, const DistDesc D, uint32_t *a) {
    for (uint64_t col = (uint64_t)blockIdx.x * kDistThreads + threadIdx.x; col < D.slice; col += (uint64_t)gridDim.x * kDistThreads) {
        const uint32_t y = (uint32_t)(col / D.nx), x = (uint32_t)(col - (uint64_t)y * D.nx);
        uint32_t steps = kDistInf;
        for (uint32_t z = 0; z < D.nz; z++) {
            const uint64_t i = col + (uint64_t)z * D.slice;
            steps = dist_step_advance(steps, target(D, x, y, z, i));
            a[i] = steps;
        }
        uint32_t back = kDistInf;
        for (uint32_t z = D.nz; z-- > 0u;) {
            const uint64_t i = col + (uint64_t)z * D.slice;
            const uint32_t below = a[i];
            back = dist_step_advance(back, below == 0u);
            a[i] = dist_steps_squared(below < back ? below : back, D.w[2]);
        }
    }
}

template <int AXIS>  // 0: along x, 1: along y
__global__ __launch_bounds__(kDistThreads) void dist_line_kernel(const DistDesc D, const uint32_t *g, uint32_t *stack, uint32_t *out) {
    const uint64_t lines = (AXIS == 1 ? (uint64_t)D.nx : (uint64_t)D.ny) * D.nz;
    for (uint64_t line = (uint64_t)blockIdx.x * kDistThreads + threadIdx.x; line < lines; line += (uint64_t)gridDim.x * kDistThreads) {
        if constexpr (AXIS == 1) {
            const uint64_t z = line / D.nx, x = line - z * D.nx;
            (void)dist_line(g, stack, out, x + z * D.slice, D.nx, D.ny, D.w[1]);
        } else {
            (void)dist_line(g, stack, out, line * D.nx, 1u, D.nx, D.w[0]);
        }
    }
}

// out[z][x][y] = in[z][y][x]: a workgroup moves tiles of 32 x 32 entries through LDS, reading rows of x and writing rows of y, 8 rows a trip.
// nx, ny: the extents of `in`.  The tile's rows are padded to 33 words: a column read meets 32 different banks.
constexpr uint32_t kDistTile = 32, kDistTileRows = kDistThreads / kDistTile;
__global__ __launch_bounds__(kDistThreads) void dist_transpose_kernel(uint32_t nx, uint32_t ny, uint32_t nz, const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
    __shared__ uint32_t tile[kDistTile][kDistTile + 1u];
    const uint32_t tx = (nx + kDistTile - 1u) / kDistTile, ty = (ny + kDistTile - 1u) / kDistTile;
    const uint64_t tiles = (uint64_t)tx * ty * nz, slice = (uint64_t)nx * ny;
    const uint32_t lx = threadIdx.x % kDistTile, ly = threadIdx.x / kDistTile;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // block-uniform
        const uint64_t row = t / tx, z = row / ty;
        const uint32_t x0 = (uint32_t)(t - row * tx) * kDistTile, y0 = (uint32_t)(row - z * ty) * kDistTile;
        for (uint32_t r = ly; r < kDistTile; r += kDistTileRows)
            if (x0 + lx < nx && y0 + r < ny) tile[r][lx] = in[z * slice + (uint64_t)(y0 + r) * nx + x0 + lx];
        __syncthreads();
        for (uint32_t r = ly; r < kDistTile; r += kDistTileRows)
            if (y0 + lx < ny && x0 + r < nx) out[z * slice + (uint64_t)(x0 + r) * ny + y0 + lx] = tile[lx][r];
        __syncthreads();  // the next tile's load overwrites this one
    }
}

constexpr uint32_t kDistStatsWords = 2, kDistMaskWords = 4;

// partial[2 b]: the zeros workgroup b saw; partial[2 b + 1]: the largest value that is not INF (0: none)
__global__ __launch_bounds__(kDistThreads) void dist_stats_kernel(const DistDesc D, const uint32_t *__restrict__ a, unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_zeros;
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) { s_zeros = 0ull; s_max = 0u; }
    __syncthreads();
    uint32_t zeros = 0u, top = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * kDistThreads + threadIdx.x; i < D.n; i += (uint64_t)gridDim.x * kDistThreads) {
        const uint32_t v = a[i];
        zeros += v == 0u;
        if (v != kDistInf && v > top) top = v;
    }
    block_add(&s_zeros, zeros);
    top = wave_reduce(top, WaveMax());
    if ((threadIdx.x & (warpSize - 1)) == 0 && top) atomicMax(&s_max, top);
    __syncthreads();
    if (threadIdx.x == 0) { partial[2u * blockIdx.x] = s_zeros; partial[2u * blockIdx.x + 1u] = s_max; }
}

// partial[4 b + ...]: |S|, |M|, |M \ S|, |S \ M| over workgroup b's voxels.  out: NULL when only the counts are asked for.
template <int VOL>
__global__ __launch_bounds__(kDistThreads) void dist_mask_kernel(const DistVolumeTarget<VOL> S, const DistDesc D, const uint32_t *__restrict__ a, void *__restrict__ out,
                                                                 unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long s_n[kDistMaskWords];
    if (threadIdx.x < kDistMaskWords) s_n[threadIdx.x] = 0ull;
    __syncthreads();
    uint32_t n_s = 0u, n_m = 0u, n_add = 0u, n_rem = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * kDistThreads + threadIdx.x; i < D.n; i += (uint64_t)gridDim.x * kDistThreads) {
        uint32_t x, y, z;
        label_coords((uint32_t)i, D.nx, D.ny, x, y, z);
        const bool in_s = S.in_set(D, x, y, z), in_m = dist_in_result(a[i], D.r2, D.above != 0u);
        n_s += in_s; n_m += in_m; n_add += in_m && !in_s; n_rem += in_s && !in_m;
        if (!out) continue;
        const uint32_t bits = in_m == in_s ? voxel_texel_bits<VOL>(S.V, x, y, z) : (in_m ? D.fill_in_bits : D.fill_out_bits);
        store_texel_bits<texel_class(VOL)>(out, i, bits);
    }
    block_add(&s_n[0], n_s); block_add(&s_n[1], n_m); block_add(&s_n[2], n_add); block_add(&s_n[3], n_rem);
    publish_partials<kDistMaskWords>(partial, s_n);
}

// ---- a round's launches, written once: vk_distance_transform brackets them with its timing phases, dist_launch_inside (vk_dist_launch.hpp)
// runs them for another pass ----
struct DistGrids { uint32_t column, y, x, tile, voxel; };
static DistGrids dist_grids(const vk_ctx *ctx, const DistDesc &D) {
    auto blocks_for = [&](uint64_t items) { return label_blocks((items + kDistThreads - 1u) / kDistThreads, ctx->dist_max_blocks); };
    DistGrids G;
    G.column = blocks_for(D.slice); G.y = blocks_for((uint64_t)D.nx * D.nz); G.x = blocks_for((uint64_t)D.ny * D.nz);
    G.tile = label_blocks((uint64_t)((D.nx + kDistTile - 1u) / kDistTile) * ((D.ny + kDistTile - 1u) / kDistTile) * D.nz, ctx->dist_max_blocks);
    G.voxel = std::min<uint32_t>(blocks_for(D.n), kPassMaxPartials);  // the counting kernels: a partial result per workgroup
    return G;
}
// the columns of the volume's predicate into a
static void dist_launch_column(vk_ctx *ctx, const VolumeDesc &V, const DistDesc &D, const DistGrids &G, uint32_t *a) {
    with_scalar_kind(ctx->vol_kind, [&](auto VOL) {
        hipLaunchKernelGGL(dist_column_kernel<DistVolumeTarget<VOL()>>, dim3(G.column), dim3(kDistThreads), 0, ctx->stream, DistVolumeTarget<VOL()>{V}, D, a);
    });
}
// a -> b along y
static void dist_launch_line_y(vk_ctx *ctx, const DistDesc &D, const DistGrids &G, uint32_t *a, uint32_t *b, uint32_t *stack) {
    hipLaunchKernelGGL(dist_line_kernel<1>, dim3(G.y), dim3(kDistThreads), 0, ctx->stream, D, (const uint32_t *)a, stack, b);
}
// b -> a along x: b is transposed into a, slice by slice, the y kernel runs on the volume with x and y exchanged (a -> b), and b is transposed
// back into a; under dist_x_plain the line function runs along the rows instead
static void dist_launch_line_x(vk_ctx *ctx, const DistDesc &D, const DistGrids &G, uint32_t *a, uint32_t *b, uint32_t *stack) {
    if (ctx->dist_x_plain) {
        hipLaunchKernelGGL(dist_line_kernel<0>, dim3(G.x), dim3(kDistThreads), 0, ctx->stream, D, (const uint32_t *)b, stack, a);
        return;
    }
    DistDesc Dt = D;
    Dt.nx = D.ny; Dt.ny = D.nx; Dt.w[0] = D.w[1]; Dt.w[1] = D.w[0];
    hipLaunchKernelGGL(dist_transpose_kernel, dim3(G.tile), dim3(kDistThreads), 0, ctx->stream, D.nx, D.ny, D.nz, (const uint32_t *)b, a);
    hipLaunchKernelGGL(dist_line_kernel<1>, dim3(G.x), dim3(kDistThreads), 0, ctx->stream, Dt, (const uint32_t *)a, stack, b);
    hipLaunchKernelGGL(dist_transpose_kernel, dim3(G.tile), dim3(kDistThreads), 0, ctx->stream, D.ny, D.nx, D.nz, (const uint32_t *)b, a);
}

void dist_launch_inside(vk_ctx *ctx, const vk_voxel_box &B, float lo_k, float hi_k, const uint32_t spacing[3], uint32_t *a, uint32_t *b, uint32_t *stack) {
    DistDesc D{};
    D.nx = ctx->nx; D.ny = ctx->ny; D.nz = ctx->nz;
    D.n = (uint64_t)ctx->nx * ctx->ny * ctx->nz; D.slice = (uint64_t)ctx->nx * ctx->ny;
    for (int c = 0; c < 3; c++) D.w[c] = spacing[c];
    D.complement = 1u;
    D.box = B;
    D.lo_k = lo_k; D.hi_k = hi_k;
    const DistGrids G = dist_grids(ctx, D);
    dist_launch_column(ctx, volume_desc(ctx), D, G, a);
    dist_launch_line_y(ctx, D, G, a, b, stack);
    dist_launch_line_x(ctx, D, G, a, b, stack);
}

extern "C" {

int vk_distance_transform(vk_ctx *ctx, const vk_distance_request *req, const vk_voxel_box *box, uint32_t *d2_out, void *dense_out, vk_distance_result *result) {
    static const char *const entry = "vk_distance_transform";
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = dist_validate(req, d2_out != nullptr, dense_out != nullptr, result != nullptr)) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + why);
    const bool install = (req->flags & VK_DIST_INSTALL) != 0u;
    if (int rc = pass_install_refused(ctx, entry, "VK_DIST_INSTALL", install)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, entry, "distance")) return rc;
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, entry, "VK_DIST_CLIP_BOX", box, (req->flags & VK_DIST_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, entry, "distance")) return rc;
    const uint64_t n = (uint64_t)ctx->nx * ctx->ny * ctx->nz;
    if (n > kDistMaxVoxels) return fail(ctx, VK_ERR_UNSUPPORTED, "distance: a volume of more than 2^32 - 2 voxels (voxel indices are 32-bit)");
    if (!dist_d2_fits(req->spacing, ctx->nx, ctx->ny, ctx->nz))
        return fail(ctx, VK_ERR_UNSUPPORTED, "distance: sum_c (spacing[c] (n_c - 1))^2 exceeds 0xFFFFFFFE: a squared distance would not fit in 32 bits");

    const int kind = ctx->vol_kind;
    const bool morph = dist_is_morph(req->op);
    DistDesc D{};
    D.nx = ctx->nx; D.ny = ctx->ny; D.nz = ctx->nz;
    D.above = dist_result_is_above(req->op) ? 1u : 0u;
    D.n = n; D.slice = (uint64_t)ctx->nx * ctx->ny;
    D.r2 = dist_r2(req->radius);
    for (int c = 0; c < 3; c++) D.w[c] = req->spacing[c];
    D.complement = dist_first_target_is_complement(req->op) ? 1u : 0u;
    D.box = B;
    D.lo_k = label_scale_bound(req->lo, ctx->format);
    D.hi_k = label_scale_bound(req->hi, ctx->format);
    D.fill_in_bits = label_fill_bits(req->fill_in, ctx->format);
    D.fill_out_bits = label_fill_bits(req->fill_out, ctx->format);
    const DistGrids G = dist_grids(ctx, D);
    const uint32_t column_blocks = G.column, voxel_blocks = G.voxel;

    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, entry};
    // (debug, vk_debug_set_param("dist_timing", k): phase k alone between the context's timer events, read with vk_timer_elapsed_ms --
    //  1 column, 2 line y, 3 line x of the first round, 4 .. 6 of the second, 7 stats or mask)
    const uint32_t timing = ctx->dist_timing;

    const size_t dense_bytes = pass_dense_bytes(ctx->format, n);
    DeviceTemp d_a, d_b, d_stack, d_partial, d_out;
    if (int rc = call.alloc(d_a, (size_t)n * 4u, "the distance array")) return rc;
    if (int rc = call.alloc(d_b, (size_t)n * 4u, "the second distance array")) return rc;
    if (int rc = call.alloc(d_stack, (size_t)n * 4u, "the envelope stacks")) return rc;
    PassPartials sums(voxel_blocks, morph ? kDistMaskWords : kDistStatsWords);
    if (int rc = call.alloc(d_partial, sums.bytes(), "the partial counts")) return rc;
    if (dense_out || install)
        if (int rc = call.alloc(d_out, dense_bytes, "the output buffer")) return rc;
    uint32_t *a = (uint32_t *)d_a.p, *b = (uint32_t *)d_b.p, *stack = (uint32_t *)d_stack.p;
    unsigned long long *partial = (unsigned long long *)d_partial.p;

    // a round: the columns of the target into a, then a -> b along y and b -> a along x
    auto lines = [&](uint32_t k) {
        call.phase(timing == k + 1u, [&] { dist_launch_line_y(ctx, D, G, a, b, stack); });
        call.phase(timing == k + 2u, [&] { dist_launch_line_x(ctx, D, G, a, b, stack); });
    };
    call.phase(timing == 1u, [&] { dist_launch_column(ctx, V, D, G, a); });
    lines(1u);
    if (dist_two_rounds(req->op)) {
        call.phase(timing == 4u, [&] { hipLaunchKernelGGL(dist_column_kernel<DistAboveTarget>, dim3(column_blocks), dim3(kDistThreads), 0, ctx->stream, DistAboveTarget{a}, D, a); });
        lines(4u);
    }
    call.phase(timing == 7u, [&] {
        if (!morph) hipLaunchKernelGGL(dist_stats_kernel, dim3(voxel_blocks), dim3(kDistThreads), 0, ctx->stream, D, (const uint32_t *)a, partial);
        else
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(dist_mask_kernel<VOL()>, dim3(voxel_blocks), dim3(kDistThreads), 0, ctx->stream, DistVolumeTarget<VOL()>{V}, D, (const uint32_t *)a, d_out.p, partial);
            });
    });

    sums.download(call, partial);
    call.download(d2_out, a, (size_t)n * 4u);
    call.download(dense_out, d_out.p, dense_bytes);
    if (int rc = call.finish()) return rc;
    if (result) {
        vk_distance_result r{};
        if (morph) {
            r.n_foreground = sums.sum(0u); r.n_result = sums.sum(1u); r.n_added = sums.sum(2u); r.n_removed = sums.sum(3u);
        } else {
            const uint64_t zeros = sums.sum(0u);
            r.max_d2 = (uint32_t)sums.max(1u);
            r.n_foreground = r.n_result = D.complement ? n - zeros : zeros;  // D2 is 0 exactly on the target
        }
        *result = r;
    }
    return install ? call.install(d_out, D.nx, D.ny, D.nz, ctx->format, ctx->layout) : VK_OK;
}

}  // extern "C"
