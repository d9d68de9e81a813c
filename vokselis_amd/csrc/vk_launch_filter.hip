// vk_launch_filter.hip -- the volume filter pass (vk_volume_filter, vk_filter_gaussian): the stored volume into another
// volume of the same dimensions and format, a separable convolution or a 3x3x3 median.  The project's first neighbourhood kernels that
// are not a ray: LDS-tiled stencils.  Tile shapes, grid arithmetic, the clamp, the store rule, the totalOrder key, the selection network
// and the request's validation are vk_filter.hpp's, shared with the host fuzz.
//
// Convolve.  One fused kernel per volume kind and tile class (vk_filter.hpp: kFilterTiles, chosen by the largest radius).  A 256-thread
// workgroup owns an output tile and takes tiles blockIdx.x, blockIdx.x + gridDim.x, ...  It loads the tile and the halo of (rx, ry, rz)
// voxels per side as f32 into LDS, indices clamped to the volume, lanes along x; then runs the x, y and z passes in LDS.  A pass is done
// in place: every lane forms its results in registers, a barrier, the lanes write them, a barrier -- one buffer serves all three.  The x
// pass covers the rows of the y and z halo, the y pass the planes of the z halo, the z pass the tile, whose results go from registers
// through the store rule to memory.  An axis with radius 0 has no halo and no pass.  In every pass the 32 lanes of a half wave are 32
// consecutive x of one row: consecutive banks whatever the pitch; the pitch is odd, so the two halves start in different banks.
// Median.  The same tiling with halo 1, keys of 16 bits in LDS (the value, or the totalOrder key of a half); a lane selects the 14th of
// its 27 keys with the min / max network of vk_filter.hpp, in registers.
// Reading.  A texel is read by its voxel index (vk_texel.hpp: voxel_texel_bits): LINEAR one element, lanes along x coalesced; the cell
// layouts one tap of the even cell that holds the voxel (the cell of an even low corner holds 8 voxels of its own), a narrow load the
// neighbouring lanes share lines with.
//
// Loop bounds are block-uniform wherever a barrier stands.  Plain C++; no inline assembly.
#include "vk_launch.hpp"
#include "vk_filter.hpp"
#include "vk_texel.hpp"

using namespace vk;

struct FilterDesc {
    uint32_t nx, ny, nz;
    uint32_t rx, ry, rz;
    uint32_t ntx, nty;  // tiles along x and y
    uint64_t tiles;
    float w[3][2 * VK_FILTER_MAX_RADIUS + 1];
    uint32_t pad;
};
static_assert(sizeof(FilterDesc) % 8 == 0 && pass_kernargs_fit<FilterDesc>, "filter kernels: VolumeDesc + FilterDesc");

template <int FMT>
__device__ __forceinline__ uint32_t filter_store_rule(float v) {
    if constexpr (FMT == TEXEL_U8) return filter_store_unorm(v, 255.0f);
    else if constexpr (FMT == TEXEL_U16) return filter_store_unorm(v, 65535.0f);
    else return filter_store_f16(v);
}

// acc = w[0] t[0]; acc = fmaf(w[k], t[k], acc), k = 1 .. 2 r; the taps `stride` elements apart
__device__ __forceinline__ float filter_taps(const float *__restrict__ w, const float *t, uint32_t r, uint32_t stride) {
    float acc = __fmul_rn(w[0], t[0]);
    for (uint32_t k = 1; k <= 2u * r; k++) acc = fmaf(w[k], t[k * stride], acc);
    return acc;
}

template <int VOL, int CLS>
__global__ __launch_bounds__(kFilterThreads, 2) void filter_convolve_kernel(const VolumeDesc V, const FilterDesc D, void *__restrict__ out) {
    constexpr FilterTile T = kFilterTiles[CLS];
    constexpr uint32_t PX = filter_pitch_x(T), PY = filter_rows(T), PZ = filter_planes(T);
    constexpr int FMT = texel_class(VOL);
    constexpr uint32_t KX = filter_per_thread(T.tx * PY * PZ), KY = filter_per_thread(T.tx * T.ty * PZ), KZ = filter_per_thread(T.tx * T.ty * T.tz);
    __shared__ float lds[PX * PY * PZ];
    const uint32_t rx = D.rx, ry = D.ry, rz = D.rz;
    const uint32_t hx = T.tx + 2u * rx, hy = T.ty + 2u * ry, hz = T.tz + 2u * rz;  // the halo box, within (PX - 1) x PY x PZ
    const uint32_t mx = filter_div_magic(hx), my = filter_div_magic(hy);            // (block-uniform: the index arithmetic below has no divide)
    for (uint64_t tile = blockIdx.x; tile < D.tiles; tile += gridDim.x) {  // block-uniform
        uint32_t x0, y0, z0;
        filter_tile_origin(tile, D.ntx, D.nty, T, x0, y0, z0);
        // the tile and its halo, clamped
        const uint32_t n_halo = hx * hy * hz;
        for (uint32_t e = threadIdx.x; e < n_halo; e += kFilterThreads) {
            const uint32_t row = filter_div(e, mx), lx = e - row * hx, lz = filter_div(row, my), ly = row - lz * hy;
            const uint32_t gx = filter_clamp((int64_t)x0 + lx - rx, D.nx), gy = filter_clamp((int64_t)y0 + ly - ry, D.ny), gz = filter_clamp((int64_t)z0 + lz - rz, D.nz);
            const uint32_t bits = voxel_texel_bits<VOL>(V, gx, gy, gz);
            lds[filter_lds_index(T, lx, ly, lz)] = texel_f32<VOL>(bits);
        }
        __syncthreads();
        if (rx) {  // x: tile columns, every row of the y and z halo; the result of column lx at lx + rx
            float acc[KX];
            const uint32_t n = T.tx * hy * hz;
#pragma unroll
            for (uint32_t k = 0; k < KX; k++) {
                const uint32_t e = threadIdx.x + k * kFilterThreads;
                if (e < n) {
                    const uint32_t row = e / T.tx, lx = e - row * T.tx, lz = filter_div(row, my), ly = row - lz * hy;
                    acc[k] = filter_taps(D.w[0], lds + filter_lds_index(T, lx, ly, lz), rx, 1u);
                }
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < KX; k++) {
                const uint32_t e = threadIdx.x + k * kFilterThreads;
                if (e < n) {
                    const uint32_t row = e / T.tx, lx = e - row * T.tx, lz = filter_div(row, my), ly = row - lz * hy;
                    lds[filter_lds_index(T, lx + rx, ly, lz)] = acc[k];
                }
            }
            __syncthreads();
        }
        if (ry) {  // y: tile columns and rows, every plane of the z halo; the result of row ly at ly + ry
            float acc[KY];
            const uint32_t n = T.tx * T.ty * hz;
#pragma unroll
            for (uint32_t k = 0; k < KY; k++) {
                const uint32_t e = threadIdx.x + k * kFilterThreads;
                if (e < n) {
                    const uint32_t row = e / T.tx, lx = e - row * T.tx, lz = row / T.ty, ly = row - lz * T.ty;
                    acc[k] = filter_taps(D.w[1], lds + filter_lds_index(T, lx + rx, ly, lz), ry, PX);
                }
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < KY; k++) {
                const uint32_t e = threadIdx.x + k * kFilterThreads;
                if (e < n) {
                    const uint32_t row = e / T.tx, lx = e - row * T.tx, lz = row / T.ty, ly = row - lz * T.ty;
                    lds[filter_lds_index(T, lx + rx, ly + ry, lz)] = acc[k];
                }
            }
            __syncthreads();
        }
        // z: the tile, from LDS through the store rule to memory
#pragma unroll
        for (uint32_t k = 0; k < KZ; k++) {
            const uint32_t e = threadIdx.x + k * kFilterThreads;  // < tx ty tz: the tile's voxels are a multiple of the workgroup
            const uint32_t row = e / T.tx, lx = e - row * T.tx, lz = row / T.ty, ly = row - lz * T.ty;
            const float *t = lds + filter_lds_index(T, lx + rx, ly + ry, lz);
            const float v = rz ? filter_taps(D.w[2], t, rz, PX * PY) : t[0];
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            if (gx < D.nx && gy < D.ny && gz < D.nz) store_texel_bits<FMT>(out, filter_voxel_offset(gx, gy, gz, D.nx, D.ny), filter_store_rule<FMT>(v));
        }
        __syncthreads();  // the next tile's load overwrites what the z pass reads
    }
}
static_assert((kFilterTiles[0].tx * kFilterTiles[0].ty * kFilterTiles[0].tz) % kFilterThreads == 0 && (kFilterTiles[1].tx * kFilterTiles[1].ty * kFilterTiles[1].tz) % kFilterThreads == 0 &&
                  (kFilterTiles[2].tx * kFilterTiles[2].ty * kFilterTiles[2].tz) % kFilterThreads == 0 && (kMedianTile.tx * kMedianTile.ty * kMedianTile.tz) % kFilterThreads == 0,
              "a tile's voxels are a multiple of the workgroup");

template <int VOL>
__global__ __launch_bounds__(kFilterThreads) void filter_median_kernel(const VolumeDesc V, const FilterDesc D, void *__restrict__ out) {
    constexpr FilterTile T = kMedianTile;
    constexpr uint32_t PX = filter_pitch_x(T), PY = filter_rows(T), PZ = filter_planes(T);
    constexpr int FMT = texel_class(VOL);
    constexpr uint32_t HX = T.tx + 2u, HY = T.ty + 2u, HZ = T.tz + 2u;
    constexpr uint32_t KZ = filter_per_thread(T.tx * T.ty * T.tz);
    __shared__ uint16_t lds[PX * PY * PZ];
    for (uint64_t tile = blockIdx.x; tile < D.tiles; tile += gridDim.x) {  // block-uniform
        uint32_t x0, y0, z0;
        filter_tile_origin(tile, D.ntx, D.nty, T, x0, y0, z0);
        for (uint32_t e = threadIdx.x; e < HX * HY * HZ; e += kFilterThreads) {
            const uint32_t row = e / HX, lx = e - row * HX, lz = row / HY, ly = row - lz * HY;
            const uint32_t gx = filter_clamp((int64_t)x0 + lx - 1, D.nx), gy = filter_clamp((int64_t)y0 + ly - 1, D.ny), gz = filter_clamp((int64_t)z0 + lz - 1, D.nz);
            const uint32_t bits = voxel_texel_bits<VOL>(V, gx, gy, gz);
            lds[filter_lds_index(T, lx, ly, lz)] = (uint16_t)(FMT == TEXEL_F16 ? filter_f16_key(bits) : bits);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < KZ; k++) {
            const uint32_t e = threadIdx.x + k * kFilterThreads;
            const uint32_t row = e / T.tx, lx = e - row * T.tx, lz = row / T.ty, ly = row - lz * T.ty;
            uint32_t v[27];
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++)
#pragma unroll
                for (uint32_t b = 0; b < 3u; b++)
#pragma unroll
                    for (uint32_t a = 0; a < 3u; a++) v[a + 3u * b + 9u * c] = lds[filter_lds_index(T, lx + a, ly + b, lz + c)];
            const uint32_t m = filter_median27(v);
            const uint32_t gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
            if (gx < D.nx && gy < D.ny && gz < D.nz) store_texel_bits<FMT>(out, filter_voxel_offset(gx, gy, gz, D.nx, D.ny), FMT == TEXEL_F16 ? filter_f16_unkey(m) : m);
        }
        __syncthreads();  // the next tile's load overwrites the keys
    }
}

template <int VOL>
static void filter_launch_convolve(vk_ctx *ctx, uint32_t cls, uint32_t grid, const VolumeDesc &V, const FilterDesc &D, void *out) {
    switch (cls) {
        case 0: hipLaunchKernelGGL((filter_convolve_kernel<VOL, 0>), dim3(grid), dim3(kFilterThreads), 0, ctx->stream, V, D, out); break;
        case 1: hipLaunchKernelGGL((filter_convolve_kernel<VOL, 1>), dim3(grid), dim3(kFilterThreads), 0, ctx->stream, V, D, out); break;
        default: hipLaunchKernelGGL((filter_convolve_kernel<VOL, 2>), dim3(grid), dim3(kFilterThreads), 0, ctx->stream, V, D, out); break;
    }
}

extern "C" {

int vk_volume_filter(vk_ctx *ctx, const struct vk_volume_filter *f, void *dense_out) {
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = filter_validate(f, dense_out != nullptr)) return fail(ctx, VK_ERR_INVALID, std::string("vk_volume_filter: ") + why);
    const bool install = (f->flags & VK_FILTER_INSTALL) != 0u;
    if (int rc = pass_install_refused(ctx, "vk_volume_filter", "VK_FILTER_INSTALL", install)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, "vk_volume_filter", "filter")) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, "vk_volume_filter", "filter")) return rc;

    const int kind = ctx->vol_kind;
    const bool median = f->op == VK_FILTER_MEDIAN3;
    FilterDesc D{};
    D.nx = ctx->nx; D.ny = ctx->ny; D.nz = ctx->nz;
    uint32_t rmax = 0u;
    if (!median) {
        D.rx = f->radius[0]; D.ry = f->radius[1]; D.rz = f->radius[2];
        for (int a = 0; a < 3; a++) {
            rmax = f->radius[a] > rmax ? f->radius[a] : rmax;
            for (uint32_t k = 0; f->radius[a] && k <= 2u * f->radius[a]; k++) D.w[a][k] = f->weights[a][k];
        }
    }
    const uint32_t cls = filter_class(rmax);
    const FilterGrid G = filter_grid(D.nx, D.ny, D.nz, median ? kMedianTile : kFilterTiles[cls], ctx->filter_max_blocks);
    D.ntx = G.ntx; D.nty = G.nty; D.tiles = G.tiles;

    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, "vk_volume_filter"};
    const size_t bytes = pass_dense_bytes(ctx->format, (uint64_t)D.nx * D.ny * D.nz);
    DeviceTemp d_out;
    if (int rc = call.alloc(d_out, bytes, "the output buffer")) return rc;
    // (debug, vk_debug_set_param("filter_timing", 1): the kernel alone between the context's timer events, read with vk_timer_elapsed_ms)
    call.phase(ctx->filter_timing != 0u, [&] {
        with_scalar_kind(kind, [&](auto VOL) {
            if (median) hipLaunchKernelGGL(filter_median_kernel<VOL()>, dim3(G.blocks), dim3(kFilterThreads), 0, ctx->stream, V, D, d_out.p);
            else filter_launch_convolve<VOL()>(ctx, cls, G.blocks, V, D, d_out.p);
        });
    });
    call.download(dense_out, d_out.p, bytes);
    if (int rc = call.finish(dense_out || !install)) return rc;  // an install alone is not waited for
    return install ? call.install(d_out, D.nx, D.ny, D.nz, ctx->format, ctx->layout) : VK_OK;
}

int vk_filter_gaussian(double sigma_voxels, uint32_t radius, float *weights) {
    if (const char *why = filter_gaussian(sigma_voxels, radius, weights)) return fail(nullptr, VK_ERR_INVALID, std::string("vk_filter_gaussian: ") + why);
    return VK_OK;
}

}  // extern "C"
