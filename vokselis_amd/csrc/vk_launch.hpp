// vk_launch.hpp -- host side of the vk_launch_*.hip files (included by them, and by vk_render.hip for has_table_layout): the runtime choices that
// select a kernel instantiation, each written once.  A helper turns its runtime values into compile-time tags and hands them to a generic lambda that names the kernel:
//     with_out_count(ctx, count, [&](auto OUT, auto COUNT) { hipLaunchKernelGGL((kernel<..., OUT(), COUNT()>), ...); });
// A helper calls its lambda with exactly the combinations the ladder it replaces spelled out: the set of instantiated kernels is the same.
#pragma once

#include "vk_ctx.hpp"

#include <type_traits>

namespace vk {

// The by-value arguments of a march kernel -- LaunchDesc, VolumeDesc and the family's own descriptors -- share the 4 KiB kernel-argument
// segment with the hidden arguments the runtime appends (at most 256 bytes): the sum is held here, not each struct on its own.
template <class... D>
constexpr bool kernargs_fit = sizeof(LaunchDesc) + sizeof(VolumeDesc) + (sizeof(D) + ... + 0) + 256 <= 4096;
static_assert(kernargs_fit<>, "raymarch_naive_kernel, the compute kernels: LaunchDesc + VolumeDesc");
static_assert(kernargs_fit<StagedDesc>, "the staged kernels: LaunchDesc + VolumeDesc + StagedDesc");
static_assert(kernargs_fit<TfDesc, ClipDesc>, "raymarch_tf_kernel, raymarch_mip_kernel and their _clip_ kernels: LaunchDesc + VolumeDesc + TfDesc (+ ClipDesc)");
static_assert(kernargs_fit<TfDesc, LightDesc, ClipDesc>, "raymarch_lit_kernel, raymarch_lit_clip_kernel: LaunchDesc + VolumeDesc + TfDesc + LightDesc (+ ClipDesc)");
static_assert(kernargs_fit<IsoDesc, ClipDesc>, "raymarch_iso_kernel, raymarch_iso_clip_kernel: LaunchDesc + VolumeDesc + IsoDesc (+ ClipDesc)");
static_assert(kernargs_fit<IsoDesc, GeomDesc, ClipDesc>, "raymarch_geom_kernel, raymarch_u16_geom_kernel and their _clip_ kernels: LaunchDesc + VolumeDesc + IsoDesc + GeomDesc (+ ClipDesc)");

template <int I>
using int_tag = std::integral_constant<int, I>;
template <bool B>
using bool_tag = std::integral_constant<bool, B>;

// f(OUT): the context's output format
template <class F>
void with_out(const vk_ctx *ctx, F &&f) {
    if (ctx->out_format == VK_OUT_RGBA16F) f(int_tag<OUT_RGBA16F>()); else f(int_tag<OUT_RGBA32F>());
}

// f(OUT, COUNT)
template <class F>
void with_out_count(const vk_ctx *ctx, bool count, F &&f) {
    with_out(ctx, [&](auto OUT) { if (count) f(OUT, bool_tag<true>()); else f(OUT, bool_tag<false>()); });
}

// f(SKIP, SAFE)
template <class F>
void with_skip_safe(bool skip, bool safe, F &&f) {
    if (skip) { if (safe) f(bool_tag<true>(), bool_tag<true>()); else f(bool_tag<true>(), bool_tag<false>()); }
    else { if (safe) f(bool_tag<false>(), bool_tag<true>()); else f(bool_tag<false>(), bool_tag<false>()); }
}

// the layouts that have table, maximum-projection and isosurface kernels: dispatch_march refuses the others under any of the three
inline bool has_table_layout(int k) { return k == VOL_LINEAR_U8 || k == VOL_LINEAR_F16 || k == VOL_P8 || k == VOL_P16 || k == VOL_PF16 || is_u16_kind(k); }

// f(VOL, SKIP, SAFE) over the layouts that have table kernels (has_table_layout): the cell layouts in all four
// variants, the LINEAR layouts without a skip map and with clamped indices only.
template <class F>
void with_table_layout(const vk_ctx *ctx, bool skip, bool safe, F &&f) {
    auto cells = [&](auto VOL) { with_skip_safe(skip, safe, [&](auto SKIP, auto SAFE) { f(VOL, SKIP, SAFE); }); };
    switch (ctx->vol_kind) {
        case VOL_P8: cells(int_tag<VOL_P8>()); break;
        case VOL_P16: cells(int_tag<VOL_P16>()); break;
        case VOL_PF16: cells(int_tag<VOL_PF16>()); break;
        case VOL_LINEAR_F16: f(int_tag<VOL_LINEAR_F16>(), bool_tag<false>(), bool_tag<true>()); break;
        default: f(int_tag<VOL_LINEAR_U8>(), bool_tag<false>(), bool_tag<true>()); break;
    }
}

// Dynamic LDS of a cell kernel (vk_march_kernel_body.hpp) -- the fast path of the cell layouts keeps its per-axis index tables there
// (vk_march.hpp: load_cell_luts) -- and, for the variants without skipping, V.lut moved on to the byte-offset copy of the tables.
// SPECKLE: the kernel decodes lone-speckle codes (the built-in skip kernels of the u8 cell layouts, but for probe-ahead) and keeps the corners' table behind them.
template <int VOL, bool SKIP, bool SAFE, bool SPECKLE = false>
uint32_t cell_kernel_lds(const vk_ctx *ctx, VolumeDesc &V) {
    if (!SKIP && V.lut) V.lut += cell_lut_entries(V.nx, V.ny, V.nz);
    constexpr bool lut = is_cell_layout(VOL) && !SAFE;
    constexpr bool corners = lut && SKIP && SPECKLE && (VOL == VOL_P8 || VOL == VOL_P16);
    return (lut ? cell_lut_bytes(V.nx, V.ny, V.nz) : 0u) + (corners ? kSpeckleLutBytes : 0u) + ctx->naive_lds_pad;  // (pad: occupancy experiments, vk_debug_set_param)
}

}  // namespace vk
