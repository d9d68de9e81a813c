// vk_filter.hpp -- the volume filter pass (vk_volume_filter, vk_filter_gaussian): the validation of a caller's
// vk_volume_filter, the Gaussian weights, the tile shapes and their LDS extents, the grid and tile arithmetic, the clamp, the store rule
// of the three formats, the totalOrder key of an f16 and the selection network of the median, shared by the kernels and their host
// (vk_launch_filter.hip) and the host fuzz (tests/filter_fuzz.cpp, plain g++ under ASan / UBSan).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vokselis_hip.h"
#include "vk_box.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VK_FILTER_HD __host__ __device__ __forceinline__
#else
#define VK_FILTER_HD inline
#endif

namespace vk {

// ---- the request -------------------------------------------------------------------------------------------------------------
// A caller's request.  Returns nullptr, or what is wrong (VK_ERR_INVALID).  have_out: dense_out is not NULL.
inline const char *filter_validate(const struct vk_volume_filter *f, bool have_out) {
    if (!f) return "the request is NULL";
    if (f->op != VK_FILTER_CONVOLVE && f->op != VK_FILTER_MEDIAN3) return "unknown op (VK_FILTER_CONVOLVE, VK_FILTER_MEDIAN3)";
    if (f->flags & ~(uint32_t)VK_FILTER_INSTALL) return "unknown flag (VK_FILTER_INSTALL)";
    if (f->op == VK_FILTER_CONVOLVE) {
        for (int a = 0; a < 3; a++) {
            if (f->radius[a] > (uint32_t)VK_FILTER_MAX_RADIUS) return "a radius is above VK_FILTER_MAX_RADIUS";
            if (f->radius[a] == 0u) continue;  // the axis is skipped: its weights are not read
            for (uint32_t k = 0; k <= 2u * f->radius[a]; k++)
                if (!(fabsf(f->weights[a][k]) <= VK_FILTER_MAX_WEIGHT)) return "a used weight is not finite or beyond +-VK_FILTER_MAX_WEIGHT";
        }
    }
    if (!have_out && !(f->flags & VK_FILTER_INSTALL)) return "neither dense_out nor VK_FILTER_INSTALL: the result would go nowhere";
    return nullptr;
}

// vk_filter_gaussian.  Returns nullptr, or what is wrong (VK_ERR_INVALID).
inline const char *filter_gaussian(double sigma, uint32_t radius, float *weights) {
    if (!weights) return "weights is NULL";
    if (!isfinite(sigma) || !(sigma > 0.0)) return "sigma must be finite and > 0";
    if (radius < 1u || radius > (uint32_t)VK_FILTER_MAX_RADIUS) return "radius must be in [1, VK_FILTER_MAX_RADIUS]";
    double g[2 * VK_FILTER_MAX_RADIUS + 1], sum = 0.0;
    const uint32_t n = 2u * radius + 1u;
    for (uint32_t k = 0; k < n; k++) {
        const double d = (double)k - (double)radius;
        g[k] = exp(-(d * d) / (2.0 * sigma * sigma));
    }
    for (uint32_t k = 0; k < n; k++) sum += g[k];
    for (uint32_t k = 0; k < n; k++) weights[k] = (float)(g[k] / sum);
    return nullptr;
}

// ---- tiles -------------------------------------------------------------------------------------------------------------------
// A 256-thread workgroup owns an output tile of tx x ty x tz voxels and keeps the tile and its halo of up to r voxels per side in LDS.
// The class of a request is chosen by its largest radius; the median uses the tile of its own (keys of 16 bits, halo 1).
constexpr uint32_t kFilterThreads = 256;
constexpr uint32_t kFilterMaxBlocks = 1u << 22;  // grid-stride kernels: a launch may not exceed 2^32 threads
struct FilterTile {
    uint32_t tx, ty, tz, r;
};
constexpr uint32_t kFilterClasses = 3;
constexpr FilterTile kFilterTiles[kFilterClasses] = {{32u, 8u, 8u, 2u}, {32u, 8u, 8u, 4u}, {32u, 4u, 4u, 6u}};
constexpr FilterTile kMedianTile = {32u, 8u, 8u, 1u};
VK_FILTER_HD uint32_t filter_class(uint32_t rmax) { return rmax <= 2u ? 0u : (rmax <= 4u ? 1u : 2u); }

// The LDS extents of a tile shape.  The row pitch is odd: the rows a wave reads in the y and z passes start in different banks.
constexpr uint32_t filter_pitch_x(FilterTile t) { return (t.tx + 2u * t.r) | 1u; }
constexpr uint32_t filter_rows(FilterTile t) { return t.ty + 2u * t.r; }
constexpr uint32_t filter_planes(FilterTile t) { return t.tz + 2u * t.r; }
constexpr uint32_t filter_lds_elems(FilterTile t) { return filter_pitch_x(t) * filter_rows(t) * filter_planes(t); }
constexpr uint32_t filter_lds_bytes(FilterTile t, uint32_t elem_bytes) { return filter_lds_elems(t) * elem_bytes; }
constexpr uint32_t kFilterLdsLimit = 64u * 1024u;  // two workgroups fit a CU's 160 KiB
static_assert(filter_lds_bytes(kFilterTiles[0], 4u) <= kFilterLdsLimit && filter_lds_bytes(kFilterTiles[1], 4u) <= kFilterLdsLimit &&
                  filter_lds_bytes(kFilterTiles[2], 4u) <= kFilterLdsLimit && filter_lds_bytes(kMedianTile, 2u) <= kFilterLdsLimit,
              "the static LDS of every instantiation stays within 64 KiB");
// the element of the halo box at (lx, ly, lz), lx < tx + 2 rx <= tx + 2 r (likewise y, z)
VK_FILTER_HD uint32_t filter_lds_index(FilterTile t, uint32_t lx, uint32_t ly, uint32_t lz) { return (lz * filter_rows(t) + ly) * filter_pitch_x(t) + lx; }
// items a thread takes at most in a pass over `count` elements
constexpr uint32_t filter_per_thread(uint32_t count) { return (count + kFilterThreads - 1u) / kFilterThreads; }

// n / d without a divide, for the kernels' index arithmetic: d is an extent of the halo box (1 .. 64), n an element of it (below 2^14).
// m = ceil(2^20 / d); floor(n m / 2^20) == n / d while n (m d - 2^20) < 2^20, and m d - 2^20 < d: n < 2^20 / 64.
constexpr uint32_t kFilterDivMaxD = 64u, kFilterDivMaxN = 1u << 14;
VK_FILTER_HD uint32_t filter_div_magic(uint32_t d) { return ((1u << 20) + d - 1u) / d; }
VK_FILTER_HD uint32_t filter_div(uint32_t n, uint32_t magic) { return (uint32_t)(((uint64_t)n * magic) >> 20); }
static_assert((kFilterTiles[0].tx + 2u * kFilterTiles[0].r) * filter_rows(kFilterTiles[0]) * filter_planes(kFilterTiles[0]) < kFilterDivMaxN &&
                  (kFilterTiles[1].tx + 2u * kFilterTiles[1].r) * filter_rows(kFilterTiles[1]) * filter_planes(kFilterTiles[1]) < kFilterDivMaxN &&
                  (kFilterTiles[2].tx + 2u * kFilterTiles[2].r) * filter_rows(kFilterTiles[2]) * filter_planes(kFilterTiles[2]) < kFilterDivMaxN &&
                  kFilterTiles[0].tx + 2u * kFilterTiles[0].r <= kFilterDivMaxD && kFilterTiles[1].tx + 2u * kFilterTiles[1].r <= kFilterDivMaxD &&
                  kFilterTiles[2].tx + 2u * kFilterTiles[2].r <= kFilterDivMaxD,
              "every halo box lies within filter_div's range");

// c(i, n) = min(max(i, 0), n - 1)
VK_FILTER_HD uint32_t filter_clamp(int64_t i, uint32_t n) { return i < 0 ? 0u : (i > (int64_t)n - 1 ? n - 1u : (uint32_t)i); }

// The tiles of a volume and the blocks of the launch: a block takes tiles blockIdx.x, blockIdx.x + blocks, ...
struct FilterGrid {
    uint32_t ntx, nty, ntz, blocks;
    uint64_t tiles;
};
VK_FILTER_HD FilterGrid filter_grid(uint32_t nx, uint32_t ny, uint32_t nz, FilterTile t, uint32_t max_blocks) {
    FilterGrid G;
    G.ntx = (nx + t.tx - 1u) / t.tx;
    G.nty = (ny + t.ty - 1u) / t.ty;
    G.ntz = (nz + t.tz - 1u) / t.tz;
    G.tiles = (uint64_t)G.ntx * G.nty * G.ntz;
    uint64_t b = G.tiles > kFilterMaxBlocks ? kFilterMaxBlocks : G.tiles;
    if (max_blocks && b > max_blocks) b = max_blocks;
    G.blocks = b < 1u ? 1u : (uint32_t)b;
    return G;
}
// the first voxel of tile i
VK_FILTER_HD void filter_tile_origin(uint64_t i, uint32_t ntx, uint32_t nty, FilterTile t, uint32_t &x0, uint32_t &y0, uint32_t &z0) {
    const uint64_t rest = i / ntx;
    x0 = (uint32_t)(i - rest * ntx) * t.tx;
    const uint64_t tz = rest / nty;
    y0 = (uint32_t)(rest - tz * nty) * t.ty;
    z0 = (uint32_t)tz * t.tz;
}
VK_FILTER_HD uint64_t filter_voxel_offset(uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny) { return voxel_index(x, y, z, nx, ny); }  // (the name the host fuzz checks the tiles under)

// ---- the store rule ----------------------------------------------------------------------------------------------------------
VK_FILTER_HD uint32_t filter_f32_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
#endif
}
// R8 and R16_UNORM: (uint) rintf(fminf(fmaxf(v, 0), top)), ties to even.  v is finite (the weight bound).
VK_FILTER_HD uint32_t filter_store_unorm(float v, float top) { return (uint32_t)rintf(fminf(fmaxf(v, 0.0f), top)); }
// R16F: f32 -> f16, round to nearest even, f16 denormals kept, overflow to +-inf, any NaN to 0x7E00.  Integer arithmetic: the same on
// the host and the device whatever their conversion instructions and denormal modes do.
VK_FILTER_HD uint32_t filter_store_f16(float v) {
    const uint32_t u = filter_f32_bits(v), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return 0x7e00u;
    if (a >= 0x38800000u) {  // 2^-14 and above: a normal half, or infinity
        const uint32_t m = a - 0x38000000u;
        const uint32_t h = (m + 0xfffu + ((m >> 13) & 1u)) >> 13;
        return sign | (h >= 0x7c00u ? 0x7c00u : h);
    }
    if (a < 0x33000000u) return sign;  // below 2^-25: zero
    const uint32_t e = a >> 23, mant = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;  // 14 <= shift <= 24
    uint32_t h = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (h & 1u))) h++;
    return sign | h;
}

// ---- the median --------------------------------------------------------------------------------------------------------------
// IEEE totalOrder of the stored halves as an unsigned key, and back
VK_FILTER_HD uint32_t filter_f16_key(uint32_t bits) { return (bits ^ ((bits & 0x8000u) ? 0xffffu : 0x8000u)) & 0xffffu; }
VK_FILTER_HD uint32_t filter_f16_unkey(uint32_t key) { return (key ^ ((key & 0x8000u) ? 0x8000u : 0xffffu)) & 0xffffu; }

VK_FILTER_HD void filter_cswap(uint32_t &a, uint32_t &b) {
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    a = lo;
    b = hi;
}
// the minimum of a[0 .. K) into a[0], the maximum into a[K - 1]
template <int K>
VK_FILTER_HD void filter_minmax(uint32_t *a) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < K / 2; i++) filter_cswap(a[i], a[K - 1 - i]);  // the minimum is now among a[0 .. (K + 1) / 2), the maximum among a[K / 2 .. K)
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 1; i < (K + 1) / 2; i++) filter_cswap(a[0], a[i]);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = K / 2; i < K - 1; i++) filter_cswap(a[i], a[K - 1]);
}
// One step of the selection: of the K live keys a[0 .. K) the smallest and the largest cannot be the median of what is left; they are
// dropped and the next key takes the place of the smallest.  K - 1 keys stay live.
template <int K>
VK_FILTER_HD void filter_median_step(uint32_t *a, uint32_t next) {
    filter_minmax<K>(a);
    a[0] = next;
}
// The 14th smallest of 27 keys (v is overwritten).  15 keys are live at first: the smallest of them has 14 above it, the largest 14
// below it, so neither is the 14th of 27; each step drops both and takes one more key in, down to the median of three.
VK_FILTER_HD uint32_t filter_median27(uint32_t (&v)[27]) {
    filter_median_step<15>(v, v[15]);
    filter_median_step<14>(v, v[16]);
    filter_median_step<13>(v, v[17]);
    filter_median_step<12>(v, v[18]);
    filter_median_step<11>(v, v[19]);
    filter_median_step<10>(v, v[20]);
    filter_median_step<9>(v, v[21]);
    filter_median_step<8>(v, v[22]);
    filter_median_step<7>(v, v[23]);
    filter_median_step<6>(v, v[24]);
    filter_median_step<5>(v, v[25]);
    filter_median_step<4>(v, v[26]);
    filter_minmax<3>(v);
    return v[1];
}

}  // namespace vk
