// vk_launch_resample.hip -- the resample pass (vk_volume_resample): a voxel box of the stored volume into a volume
// of other dimensions, by the nearest voxel, by trilinear interpolation or by the area-weighted mean, optionally mapped into another
// scalar format.  The rule is include/vokselis_hip.h's; the integer geometry, the per-axis tables, the value map, the store rule, the
// grid arithmetic and the request's validation are vk_resample.hpp's, shared with the host fuzz.
//
// One gather kernel per volume kind and mode.  The host turns the geometry into per-axis tables once per call (NEAREST: the index;
// LINEAR: i0, i1, f; AREA: first tap, tap count, weights) -- no divide and no double runs per voxel.  A 256-thread workgroup owns a tile
// of 64 x 4 output voxels, lanes along x: a wave's 64 stores are consecutive; a thread takes four voxels one above the other (one under AREA
// but for the unrolled ratio 2), computed without a branch between them so that their loads are in flight together.  The grid is three-dimensional, a block per tile;
// beyond 2^23 tiles or under a cap a block takes tiles blockIdx.x + t gridDim.x for t = 0 .. trips - 1, the trip count the launch's.  AREA is the fused footprint loop: z outermost, x innermost, the x sum of every
// (y, z) row of the footprint folded into the y sum, the y sum of every z plane into the z sum -- the three axis reductions of the rule
// over unrounded f32 intermediates, in registers; at ratio 2 a wave reads 128 consecutive source voxels per row, every one once.
// Reading.  A texel is read by its voxel index (vk_texel.hpp: voxel_texel_bits), as in the filter pass.  Offsets are 64-bit.
// No barrier, no LDS, no atomics, no workgroup waits for another.  Plain C++; no inline assembly.
#include "vk_launch.hpp"
#include "vk_resample.hpp"
#include "vk_texel.hpp"

#include <vector>

using namespace vk;

struct ResampleDesc {
    uint32_t x0, y0, z0;  // the box's low corner
    uint32_t nx, ny, nz;  // the output's extents
    uint32_t base[3];     // the axes' first table words
    uint32_t taps[3];     // AREA: the weights' stride
    uint32_t ntx, nty;
    uint32_t out_class;   // TexelClass of the output
    uint32_t map;         // the value map runs
    float a, b;
    uint32_t flat, pad;   // flat: a one-dimensional grid that strides over the tiles (vk_resample.hpp: resample_grid)
    uint64_t tiles, trips;
};
static_assert(sizeof(ResampleDesc) % 8 == 0 && pass_kernargs_fit<ResampleDesc>, "resample kernels: VolumeDesc + ResampleDesc");

template <int VOL>
__device__ __forceinline__ float resample_texel(const VolumeDesc &V, uint32_t x, uint32_t y, uint32_t z) {
    return texel_f32<VOL>(voxel_texel_bits<VOL>(V, x, y, z));
}

// The tile of a block in its trip: the block's index in a three-dimensional grid; in a flat one tile trip * gridDim.x + blockIdx.x, taken
// apart with two divides on the scalar unit.  false: past the last tile.
__device__ __forceinline__ bool resample_tile(uint32_t flat, uint64_t trip, uint64_t tiles, uint32_t ntx, uint32_t nty, uint32_t &bx, uint32_t &by, uint32_t &z) {
    if (!flat) { bx = blockIdx.x; by = blockIdx.y; z = blockIdx.z; return true; }
    const uint64_t tile = trip * gridDim.x + blockIdx.x;
    if (tile >= tiles) return false;
    const uint64_t rest = tile / ntx, z64 = rest / nty;
    bx = (uint32_t)(tile - rest * ntx); by = (uint32_t)(rest - z64 * nty); z = (uint32_t)z64;
    return true;
}

// One output voxel: its bits in the output format.  C > 0 (AREA): every output voxel has C taps on every axis -- an integer ratio,
// downsample by C -- so the footprint loops have constant bounds, are unrolled, and the C^3 loads of a voxel are in flight together;
// C == 0: the counts come from the tables.
template <int VOL, int MODE, int C>
__device__ __forceinline__ uint32_t resample_voxel(const VolumeDesc &V, const ResampleDesc &D, const uint32_t *__restrict__ tx, const uint32_t *__restrict__ ty, const uint32_t *__restrict__ tz,
                                                   uint32_t x, uint32_t y, uint32_t z) {
    uint32_t bits = 0u;
    float v = 0.0f;
    if constexpr (MODE == VK_RESAMPLE_NEAREST) {
        bits = voxel_texel_bits<VOL>(V, D.x0 + tx[x], D.y0 + ty[y], D.z0 + tz[z]);
        v = texel_f32<VOL>(bits);
    } else if constexpr (MODE == VK_RESAMPLE_LINEAR) {
        const uint32_t xa = D.x0 + tx[3u * x], xb = D.x0 + tx[3u * x + 1u], ya = D.y0 + ty[3u * y], yb = D.y0 + ty[3u * y + 1u], za = D.z0 + tz[3u * z], zb = D.z0 + tz[3u * z + 1u];
        const float fx = __uint_as_float(tx[3u * x + 2u]), fy = __uint_as_float(ty[3u * y + 2u]), fz = __uint_as_float(tz[3u * z + 2u]);
        const float l00 = resample_lerp(resample_texel<VOL>(V, xa, ya, za), resample_texel<VOL>(V, xb, ya, za), fx);
        const float l10 = resample_lerp(resample_texel<VOL>(V, xa, yb, za), resample_texel<VOL>(V, xb, yb, za), fx);
        const float l01 = resample_lerp(resample_texel<VOL>(V, xa, ya, zb), resample_texel<VOL>(V, xb, ya, zb), fx);
        const float l11 = resample_lerp(resample_texel<VOL>(V, xa, yb, zb), resample_texel<VOL>(V, xb, yb, zb), fx);
        v = resample_lerp(resample_lerp(l00, l10, fy), resample_lerp(l01, l11, fy), fz);
    } else if constexpr (C > 0) {  // C taps on every axis: the C^3 texels first, all loads in flight, then the sums in the rule's order
        const uint32_t kx0 = D.x0 + tx[2u * x], ky0 = D.y0 + ty[2u * y], kz0 = D.z0 + tz[2u * z];
        const uint32_t *wx = tx + 2u * D.nx + x * D.taps[0], *wy = ty + 2u * D.ny + y * D.taps[1], *wz = tz + 2u * D.nz + z * D.taps[2];
        float t[C][C][C];
#pragma unroll
        for (int c = 0; c < C; c++)
#pragma unroll
            for (int b = 0; b < C; b++)
#pragma unroll
                for (int a = 0; a < C; a++) t[c][b][a] = resample_texel<VOL>(V, kx0 + a, ky0 + b, kz0 + c);
        float accz = 0.0f;
#pragma unroll
        for (int c = 0; c < C; c++) {
            float accy = 0.0f;
#pragma unroll
            for (int b = 0; b < C; b++) {
                float accx = __fmul_rn(__uint_as_float(wx[0]), t[c][b][0]);
#pragma unroll
                for (int a = 1; a < C; a++) accx = fmaf(__uint_as_float(wx[a]), t[c][b][a], accx);
                accy = b ? fmaf(__uint_as_float(wy[b]), accx, accy) : __fmul_rn(__uint_as_float(wy[0]), accx);
            }
            accz = c ? fmaf(__uint_as_float(wz[c]), accy, accz) : __fmul_rn(__uint_as_float(wz[0]), accy);
        }
        v = accz;
    } else {
        const uint32_t kx0 = tx[2u * x], cx = tx[2u * x + 1u], ky0 = ty[2u * y], cy = ty[2u * y + 1u], kz0 = tz[2u * z], cz = tz[2u * z + 1u];  // counts: 1 .. kResampleMaxTaps
        const uint32_t *wx = tx + 2u * D.nx + x * D.taps[0], *wy = ty + 2u * D.ny + y * D.taps[1], *wz = tz + 2u * D.nz + z * D.taps[2];
        float accz = 0.0f;
        for (uint32_t c = 0; c < cz; c++) {
            float accy = 0.0f;
            for (uint32_t b = 0; b < cy; b++) {
                float accx = __fmul_rn(__uint_as_float(wx[0]), resample_texel<VOL>(V, D.x0 + kx0, D.y0 + ky0 + b, D.z0 + kz0 + c));
                for (uint32_t a = 1; a < cx; a++) accx = fmaf(__uint_as_float(wx[a]), resample_texel<VOL>(V, D.x0 + kx0 + a, D.y0 + ky0 + b, D.z0 + kz0 + c), accx);
                accy = b ? fmaf(__uint_as_float(wy[b]), accx, accy) : __fmul_rn(__uint_as_float(wy[0]), accx);
            }
            accz = c ? fmaf(__uint_as_float(wz[c]), accy, accz) : __fmul_rn(__uint_as_float(wz[0]), accy);
        }
        v = accz;
    }
    if (D.map) v = fmaf(D.a, v, D.b);
    if (MODE != VK_RESAMPLE_NEAREST || D.map)
        bits = D.out_class == TEXEL_U8 ? resample_store_unorm(v, 255.0f) : (D.out_class == TEXEL_U16 ? resample_store_unorm(v, 65535.0f) : filter_store_f16(v));
    return bits;
}

template <int VOL, int MODE, int C = 0>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const VolumeDesc V, const ResampleDesc D, const uint32_t *__restrict__ tab, void *__restrict__ out) {
    constexpr uint32_t KZ = resample_tile_z(MODE, (uint32_t)C);
    const uint32_t lx = threadIdx.x & (kResampleTileX - 1u), ly = threadIdx.x / kResampleTileX;
    const uint32_t *__restrict__ tx = tab + D.base[0], *__restrict__ ty = tab + D.base[1], *__restrict__ tz = tab + D.base[2];
    for (uint64_t trip = 0; trip < D.trips; trip++) {  // block-uniform, the launch's count
        uint32_t bx, by, bz;
        if (!resample_tile(D.flat, trip, D.tiles, D.ntx, D.nty, bx, by, bz)) continue;
        const uint32_t x = bx * kResampleTileX + lx, y = by * kResampleTileY + ly, z0 = bz * KZ;
        if (x >= D.nx || y >= D.ny) continue;
        uint32_t bits[KZ];
#pragma unroll
        for (uint32_t k = 0; k < KZ; k++) {  // past the last plane: the last plane again, not stored -- no branch between the voxels' loads
            const uint32_t z = z0 + k < D.nz ? z0 + k : D.nz - 1u;
            bits[k] = resample_voxel<VOL, MODE, C>(V, D, tx, ty, tz, x, y, z);
        }
#pragma unroll
        for (uint32_t k = 0; k < KZ; k++) {
            if (z0 + k >= D.nz) break;
            const uint64_t o = voxel_index(x, y, z0 + k, D.nx, D.ny);
            if (D.out_class == TEXEL_U8) reinterpret_cast<uint8_t *>(out)[o] = (uint8_t)bits[k];
            else reinterpret_cast<uint16_t *>(out)[o] = (uint16_t)bits[k];
        }
    }
}

// AREA, the other structure (debug, vk_debug_set_param("resample_area_passes", 1)): the three axis reductions as three
// launches through f32 intermediates of the call's own -- x over every row of the box, y over the x results, z over the y results, which
// goes through the map and the store rule.  The same sums in the same order: bit for bit the fused kernel's output.  VOL < 0: the input
// is an f32 array of in = (inx, iny, inz); otherwise the stored volume, read at the box's corner + the index.
struct ResampleAxisDesc {
    uint32_t x0, y0, z0;     // VOL >= 0: the box's low corner
    uint32_t inx, iny;       // VOL < 0: the input's row and plane extents
    uint32_t nx, ny, nz;     // this pass's output extents
    uint32_t axis;           // 0 x, 1 y, 2 z
    uint32_t base, n, taps;  // the axis's table: its first word, its output extent, the weights' stride
    uint32_t ntx, nty;
    uint32_t last;           // the z pass: map and store; otherwise f32 out
    uint32_t out_class, map;
    float a, b;
    uint32_t flat;
    uint64_t tiles, trips;
};
static_assert(sizeof(ResampleAxisDesc) % 8 == 0 && pass_kernargs_fit<ResampleAxisDesc>, "resample axis kernels: VolumeDesc + ResampleAxisDesc");

template <int VOL>
__global__ __launch_bounds__(kResampleThreads) void resample_area_axis_kernel(const VolumeDesc V, const ResampleAxisDesc D, const uint32_t *__restrict__ tab, const float *__restrict__ in,
                                                                              void *__restrict__ out) {
    const uint32_t lx = threadIdx.x & (kResampleTileX - 1u), ly = threadIdx.x / kResampleTileX;
    const uint32_t *__restrict__ t = tab + D.base;
    for (uint64_t trip = 0; trip < D.trips; trip++) {  // block-uniform, the launch's count
        uint32_t bx, by, z;
        if (!resample_tile(D.flat, trip, D.tiles, D.ntx, D.nty, bx, by, z)) continue;
        const uint32_t x = bx * kResampleTileX + lx, y = by * kResampleTileY + ly;
        if (x >= D.nx || y >= D.ny) continue;
        const uint32_t j = D.axis == 0u ? x : (D.axis == 1u ? y : z);
        const uint32_t k0 = t[2u * j], c = t[2u * j + 1u];
        const uint32_t *w = t + 2u * D.n + j * D.taps;
        float acc = 0.0f;
        for (uint32_t k = 0; k < c; k++) {
            const uint32_t sx = D.axis == 0u ? k0 + k : x, sy = D.axis == 1u ? k0 + k : y, sz = D.axis == 2u ? k0 + k : z;
            float v;
            if constexpr (VOL >= 0) v = resample_texel<VOL>(V, D.x0 + sx, D.y0 + sy, D.z0 + sz);
            else v = in[voxel_index(sx, sy, sz, D.inx, D.iny)];
            acc = k ? fmaf(__uint_as_float(w[k]), v, acc) : __fmul_rn(__uint_as_float(w[0]), v);
        }
        const uint64_t o = voxel_index(x, y, z, D.nx, D.ny);
        if (!D.last) { reinterpret_cast<float *>(out)[o] = acc; continue; }
        if (D.map) acc = fmaf(D.a, acc, D.b);
        const uint32_t bits = D.out_class == TEXEL_U8 ? resample_store_unorm(acc, 255.0f) : (D.out_class == TEXEL_U16 ? resample_store_unorm(acc, 65535.0f) : filter_store_f16(acc));
        if (D.out_class == TEXEL_U8) reinterpret_cast<uint8_t *>(out)[o] = (uint8_t)bits;
        else reinterpret_cast<uint16_t *>(out)[o] = (uint16_t)bits;
    }
}

static dim3 resample_dim3(const ResampleGrid &G) { return G.flat ? dim3(G.blocks) : dim3(G.ntx, G.nty, G.ntz); }

template <int VOL>
static void resample_launch(vk_ctx *ctx, int mode, uint32_t taps, dim3 grid, const VolumeDesc &V, const ResampleDesc &D, const uint32_t *tab, void *out) {
    if (mode == VK_RESAMPLE_AREA && taps == 2u) { hipLaunchKernelGGL((resample_kernel<VOL, VK_RESAMPLE_AREA, 2>), grid, dim3(kResampleThreads), 0, ctx->stream, V, D, tab, out); return; }
    if (mode == VK_RESAMPLE_AREA && taps == 3u) { hipLaunchKernelGGL((resample_kernel<VOL, VK_RESAMPLE_AREA, 3>), grid, dim3(kResampleThreads), 0, ctx->stream, V, D, tab, out); return; }
    if (mode == VK_RESAMPLE_AREA && taps == 4u) { hipLaunchKernelGGL((resample_kernel<VOL, VK_RESAMPLE_AREA, 4>), grid, dim3(kResampleThreads), 0, ctx->stream, V, D, tab, out); return; }
    switch (mode) {
        case VK_RESAMPLE_NEAREST: hipLaunchKernelGGL((resample_kernel<VOL, VK_RESAMPLE_NEAREST>), grid, dim3(kResampleThreads), 0, ctx->stream, V, D, tab, out); break;
        case VK_RESAMPLE_LINEAR: hipLaunchKernelGGL((resample_kernel<VOL, VK_RESAMPLE_LINEAR>), grid, dim3(kResampleThreads), 0, ctx->stream, V, D, tab, out); break;
        default: hipLaunchKernelGGL((resample_kernel<VOL, VK_RESAMPLE_AREA>), grid, dim3(kResampleThreads), 0, ctx->stream, V, D, tab, out); break;
    }
}

// Every refusal of a call, in the header's order, before anything is launched or written: VK_OK with the box and the plan, or the error set.
static int resample_prepare(vk_ctx *ctx, const vk_resample_request *req, const vk_voxel_box *box, bool have_out, vk_voxel_box &B, ResamplePlan &P) {
    if (const char *why = resample_validate(req, have_out)) return fail(ctx, VK_ERR_INVALID, std::string("resample: ") + why);
    if (int rc = pass_install_refused(ctx, "resample", "VK_RESAMPLE_INSTALL", (req->flags & VK_RESAMPLE_INSTALL) != 0u)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, "resample", "resample")) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, "resample", "resample")) return rc;
    if (int rc = pass_voxel_box(ctx, "resample", "VK_RESAMPLE_CLIP_BOX", box, (req->flags & VK_RESAMPLE_CLIP_BOX) != 0u, B)) return rc;
    int status = VK_ERR_INVALID;
    if (const char *why = resample_plan(req, B, ctx->format, ctx->layout, P, status)) return fail(ctx, status, std::string("resample: ") + why);
    return VK_OK;
}

extern "C" {

int vk_resample_output(vk_ctx *ctx, const vk_resample_request *req, const vk_voxel_box *box, vk_resample_result *result) {
    if (!ctx) return VK_ERR_INVALID;
    if (!result) return fail(ctx, VK_ERR_INVALID, "resample: result is NULL");
    vk_voxel_box B;
    ResamplePlan P;
    if (int rc = resample_prepare(ctx, req, box, true, B, P)) return rc;
    result->dims[0] = P.n[0]; result->dims[1] = P.n[1]; result->dims[2] = P.n[2];
    result->format = P.format;
    result->layout = P.layout;
    result->box = B;
    return VK_OK;
}

int vk_volume_resample(vk_ctx *ctx, const vk_resample_request *req, const vk_voxel_box *box, void *dense_out, vk_resample_result *result) {
    if (!ctx) return VK_ERR_INVALID;
    vk_voxel_box B;
    ResamplePlan P;
    if (int rc = resample_prepare(ctx, req, box, dense_out != nullptr, B, P)) return rc;
    const bool install = (req->flags & VK_RESAMPLE_INSTALL) != 0u;

    // the per-axis tables
    ResampleAxis ax[3];
    const uint32_t words = resample_table_layout(req->mode, P.nb, P.n, ax);
    std::vector<uint32_t> table(words);
    for (int a = 0; a < 3; a++) resample_table_fill(req->mode, ax[a], table.data());

    // downsample by 2, 3 or 4 on every axis: the unrolled footprint (debug, "resample_area_unroll" 0: the table-driven loops)
    const uint32_t taps = req->mode == VK_RESAMPLE_AREA && ctx->resample_area_unroll ? resample_uniform_taps(P.nb, P.n) : 0u;
    const ResampleGrid G = resample_grid(P.n[0], P.n[1], P.n[2], ctx->resample_max_blocks, resample_tile_z(req->mode, taps));
    ResampleDesc D{};
    D.x0 = B.x0; D.y0 = B.y0; D.z0 = B.z0;
    D.nx = P.n[0]; D.ny = P.n[1]; D.nz = P.n[2];
    for (int a = 0; a < 3; a++) { D.base[a] = ax[a].base; D.taps[a] = ax[a].taps; }
    D.ntx = G.ntx; D.nty = G.nty; D.trips = G.trips; D.tiles = G.tiles; D.flat = G.flat;
    D.out_class = P.format == VK_FMT_R8_UNORM ? TEXEL_U8 : (P.format == VK_FMT_R16_UNORM ? TEXEL_U16 : TEXEL_F16);
    D.map = P.map ? 1u : 0u;
    D.a = P.a; D.b = P.b;

    const int kind = ctx->vol_kind;
    const VolumeDesc V = volume_desc(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    PassCall call{ctx, "resample"};
    const size_t bytes = pass_dense_bytes(P.format, (uint64_t)D.nx * D.ny * D.nz);
    DeviceTemp d_tab, d_out;
    if (int rc = call.alloc(d_tab, (size_t)words * sizeof(uint32_t), "the axis tables")) return rc;
    if (int rc = call.alloc(d_out, bytes, "the output buffer")) return rc;
    call.e = hipMemcpy(d_tab.p, table.data(), (size_t)words * sizeof(uint32_t), hipMemcpyHostToDevice);  // blocking: the tables stand before the launch
    const bool passes = req->mode == VK_RESAMPLE_AREA && ctx->resample_area_passes != 0u;
    DeviceTemp d_t1, d_t2;  // the separate passes' intermediates: the x sums of the box's rows, the y sums of those
    if (call.e == hipSuccess && passes) {
        if (int rc = call.alloc(d_t1, (size_t)P.n[0] * P.nb[1] * P.nb[2] * sizeof(float), "the intermediates of the separate passes")) return rc;
        if (int rc = call.alloc(d_t2, (size_t)P.n[0] * P.n[1] * P.nb[2] * sizeof(float), "the intermediates of the separate passes")) return rc;
    }
    const uint32_t *tab = static_cast<const uint32_t *>(d_tab.p);
    // (debug, vk_debug_set_param("resample_timing", 1): the kernels alone, behind every allocation, between the context's timer events, read with vk_timer_elapsed_ms)
    call.phase(ctx->resample_timing == 1u, [&] {
        if (!passes) {
            with_scalar_kind(kind, [&](auto VOL) { resample_launch<VOL()>(ctx, req->mode, taps, resample_dim3(G), V, D, tab, d_out.p); });
            return;
        }
        for (uint32_t axis = 0; axis < 3u; axis++) {
            ResampleAxisDesc A{};
            A.x0 = B.x0; A.y0 = B.y0; A.z0 = B.z0;
            A.inx = P.n[0]; A.iny = axis == 1u ? P.nb[1] : P.n[1];
            A.nx = P.n[0]; A.ny = axis == 0u ? P.nb[1] : P.n[1]; A.nz = axis == 2u ? P.n[2] : P.nb[2];
            A.axis = axis; A.base = ax[axis].base; A.n = P.n[axis]; A.taps = ax[axis].taps;
            const ResampleGrid GA = resample_grid(A.nx, A.ny, A.nz, ctx->resample_max_blocks);
            A.ntx = GA.ntx; A.nty = GA.nty; A.tiles = GA.tiles; A.trips = GA.trips; A.flat = GA.flat;
            A.last = axis == 2u ? 1u : 0u;
            A.out_class = D.out_class; A.map = D.map; A.a = D.a; A.b = D.b;
            const float *in = axis == 1u ? static_cast<const float *>(d_t1.p) : static_cast<const float *>(d_t2.p);
            void *dst = axis == 0u ? d_t1.p : (axis == 1u ? d_t2.p : d_out.p);
            if (axis == 0u) with_scalar_kind(kind, [&](auto VOL) { hipLaunchKernelGGL(resample_area_axis_kernel<VOL()>, resample_dim3(GA), dim3(kResampleThreads), 0, ctx->stream, V, A, tab, in, dst); });
            else hipLaunchKernelGGL(resample_area_axis_kernel<-1>, resample_dim3(GA), dim3(kResampleThreads), 0, ctx->stream, V, A, tab, in, dst);
        }
    });
    call.download(dense_out, d_out.p, bytes);
    if (int rc = call.finish()) return rc;  // the call blocks; the tables are freed on return
    if (install)
        if (int rc = call.install(d_out, D.nx, D.ny, D.nz, P.format, P.layout)) return rc;
    if (result) {  // behind the install: the layout is the one the volume took
        result->dims[0] = D.nx; result->dims[1] = D.ny; result->dims[2] = D.nz;
        result->format = P.format;
        result->layout = install ? ctx->layout : 0;
        result->box = B;
    }
    return VK_OK;
}

}  // extern "C"
