// vk_launch.hpp -- host side of the vk_launch_*.hip files (included by them, and by vk_render.hip for has_table_layout and pass_needs): the runtime
// choices that select a kernel instantiation, each written once, and what the entry points of the passes that are not a march share (DESIGN.md
// section 23).  A helper turns its runtime values into compile-time tags and hands them to a generic lambda that names the kernel:
//     with_out_count(ctx, count, [&](auto OUT, auto COUNT) { hipLaunchKernelGGL((kernel<..., OUT(), COUNT()>), ...); });
// A helper calls its lambda with exactly the combinations the ladder it replaces spelled out: the set of instantiated kernels is the same.
#pragma once

#include "vk_box.hpp"
#include "vk_ctx.hpp"

#include <algorithm>
#include <type_traits>
#include <vector>

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
// ... and of a pass that is not a march: VolumeDesc and the pass's own descriptors, no LaunchDesc
template <class... D>
constexpr bool pass_kernargs_fit = sizeof(VolumeDesc) + (sizeof(D) + ... + 0) + 256 <= 4096;

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

// ---- the passes that are not a march (slice, histogram, mesh, filter, label, distance, resample, split, measure, thickness, geodesic,
// skeleton): kernels on the seven scalar kinds of has_table_layout ----------
// f(VOL) over those kinds.  A caller whose kernel covers fewer of them says so with `if constexpr` in its lambda: nothing else is instantiated.
template <class F>
void with_scalar_kind(int kind, F &&f) {
    switch (kind) {
        case VOL_P8: f(int_tag<VOL_P8>()); break;
        case VOL_P16: f(int_tag<VOL_P16>()); break;
        case VOL_PF16: f(int_tag<VOL_PF16>()); break;
        case VOL_PU16: f(int_tag<VOL_PU16>()); break;
        case VOL_LINEAR_F16: f(int_tag<VOL_LINEAR_F16>()); break;
        case VOL_LINEAR_U16: f(int_tag<VOL_LINEAR_U16>()); break;
        default: f(int_tag<VOL_LINEAR_U8>()); break;
    }
}

// The two refusals of such a pass, made one at a time because other checks stand between them: VK_OK, or the error set.  entry: the function's name;
// word: what the pass's kernels are called; subject: what the pass calls itself.
enum PassNeed { PASS_NEEDS_VOLUME, PASS_NEEDS_SCALAR_KIND };
inline int pass_needs(vk_ctx *ctx, PassNeed need, const char *entry, const char *word, const char *subject = "pass") {
    if (need == PASS_NEEDS_VOLUME) return ctx->format < 0 ? fail(ctx, VK_ERR_INVALID, std::string(entry) + ": no volume uploaded") : VK_OK;
    if (ctx->format == VK_FMT_RGBA16F_PAIR || !has_table_layout(ctx->vol_kind))
        return fail(ctx, VK_ERR_UNSUPPORTED, std::string(word) + ": the " + subject + " needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no " + word + " kernels)");
    return VK_OK;
}

// The voxel box of a call (histogram, mesh): the caller's, else the clip box where the request's flag (its name: flag) asks for it and
// one is set, else the whole volume.  VK_OK, or the error set.
inline int pass_voxel_box(vk_ctx *ctx, const char *entry, const char *flag, const vk_voxel_box *box, bool clip_flag, vk_voxel_box &B) {
    if (box && clip_flag) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": " + flag + " takes the box from the clip box: box must be NULL");
    if (box && !voxel_box_ok(*box, ctx->nx, ctx->ny, ctx->nz)) return fail(ctx, VK_ERR_INVALID, std::string(entry) + ": the box is inverted or leaves the volume");
    if (box) B = *box;
    else if (clip_flag && ctx->clip_on) B = voxel_clip_box(ctx->clip_lo, ctx->clip_hi, ctx->nx, ctx->ny, ctx->nz);
    else B = vk_voxel_box{0u, 0u, 0u, ctx->nx, ctx->ny, ctx->nz};
    return VK_OK;
}

// ... and of a pass that can install its dense output as the volume: not while a frame is being recorded.  flag: the request flag's name.
inline int pass_install_refused(vk_ctx *ctx, const char *prefix, const char *flag, bool install) {
    if (!install || !ctx->fif_open) return VK_OK;
    return fail(ctx, VK_ERR_INVALID, std::string(prefix) + ": " + flag + " while a frame is being recorded (call it outside vk_frame_begin / vk_frame_end)");
}

// the bytes of a dense array of n texels
inline size_t pass_dense_bytes(int format, uint64_t n) { return (size_t)n * (format == VK_FMT_R8_UNORM ? 1u : 2u); }

// The host frame of one call of such a pass, behind its refusals and hipSetDevice: one object per call.  It carries the first HIP error
// of the call; every step but alloc is skipped once there is one, and finish reports it.  prefix: what the call's messages begin with.
struct PassCall {
    vk_ctx *ctx;
    const char *prefix;
    hipError_t e = hipSuccess;

    // a temporary of the call (an empty one still gets a byte): VK_OK, or the error set.  what: the buffer, in the message's words
    int alloc(DeviceTemp &d, size_t bytes, const char *what) {
        e = ctx_alloc(ctx, &d.p, bytes ? bytes : 1u);
        if (e == hipSuccess) return VK_OK;
        return alloc_failed(ctx, e, prefix, what);
    }
    // launch(): the kernels of one phase, between the context's timer events where timed (the pass's X_timing names this phase).  A
    // launch that looks at HIP errors itself leaves the first in e.
    template <class F>
    void phase(bool timed, F &&launch) {
        if (timed && e == hipSuccess) e = hipEventRecord(ctx->ev0, ctx->stream);
        enqueue(launch);
        if (timed && e == hipSuccess) {
            e = hipEventRecord(ctx->ev1, ctx->stream);
            ctx->timing_open = false;
            ctx->timing_done = true;
        }
    }
    // launch() and the look at its HIP error, skipped once the call has one
    template <class F>
    void enqueue(F &&launch) {
        if (e == hipSuccess) { launch(); if (e == hipSuccess) e = hipGetLastError(); }
    }
    // The batched fixed-point loop of a pass whose rounds run until one changes nothing, the one place where such a pass waits for the
    // device in the middle of a call: B rounds are enqueued blind, then the host reads the W counts each left and stops at the first
    // that says it was the last; the pass sees to it that the rounds behind that one in its batch found nothing to do.  counts: B * W
    // words on the device.  round(r, slot): the launches of round r = 0, 1, ... (each behind enqueue where there are several), which add
    // to slot[0 .. W).  last(c): takes one round's counts into the caller's totals and says whether it was the last; called in the rounds'
    // order, never for a round behind the last.  budget: 0, or the most rounds to run -- the only thing that cuts a batch short.  The
    // loop is a phase of the call (timed).
    template <uint32_t B, uint32_t W, class R, class L>
    void iterate(bool timed, unsigned long long *counts, uint32_t budget, R &&round, L &&last) {
        phase(timed, [&] {
            uint32_t r = 0u;
            for (bool done = false; !done && e == hipSuccess;) {
                const uint32_t batch = budget ? std::min<uint32_t>(B, budget - r) : B;
                if (batch == 0u) break;
                unsigned long long got[B * W] = {};
                e = hipMemsetAsync(counts, 0, sizeof got, ctx->stream);
                for (uint32_t k = 0; k < batch; k++, r++) enqueue([&] { round(r, counts + (size_t)k * W); });
                download(got, counts, sizeof got);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
                for (uint32_t k = 0; k < batch && e == hipSuccess && !done; k++) done = last(got + (size_t)k * W);
            }
        });
    }
    // an output the caller may not have asked for (dst NULL), behind the kernels on the stream
    void download(void *dst, const void *src, size_t bytes) {
        if (e == hipSuccess && dst) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream);
    }
    // the stream runs dry (sync), then VK_OK, or the call's first HIP error set
    int finish(bool sync = true) {
        if (sync && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        return e == hipSuccess ? VK_OK : fail(ctx, VK_ERR_HIP, std::string(prefix) + ": " + hipGetErrorString(e));
    }
    // d_out becomes the volume: the build runs on the same stream behind the kernel, adopts or frees d_out, and commits only when it
    // stands: the old volume stays otherwise
    int install(DeviceTemp &d_out, uint32_t nx, uint32_t ny, uint32_t nz, int format, int layout) { return install_dense(ctx, d_out.release(), nx, ny, nz, format, layout); }
};

// Partial totals per workgroup (the kernels' half: vk_pass_blocks.hpp): a counting kernel runs at most kPassMaxPartials workgroups, each
// writes a row of `words` 64-bit words, and the host folds the rows.  One object per counting kernel: the bytes of its device buffer, the
// download behind the kernel and, once finish has run the stream dry, column k's total.
constexpr uint32_t kPassMaxPartials = 8192;
struct PassPartials {
    typedef unsigned long long word;
    uint32_t rows, words;  // rows: the counting kernel's workgroups
    std::vector<word> v;
    PassPartials(uint32_t rows, uint32_t words) : rows(rows), words(words), v((size_t)rows * words) {}
    size_t bytes() const { return v.size() * 8u; }
    void download(PassCall &call, const void *src) { call.download(v.data(), src, bytes()); }
    template <class OP>
    word fold(uint32_t k, word s, OP op) const {
        for (uint32_t b = 0; b < rows; b++) s = op(s, v[(size_t)words * b + k]);
        return s;
    }
    word sum(uint32_t k) const { return fold(k, 0ull, [](word a, word b) { return a + b; }); }
    word max(uint32_t k) const { return fold(k, 0ull, [](word a, word b) { return std::max(a, b); }); }
    word min(uint32_t k) const { return fold(k, ~0ull, [](word a, word b) { return std::min(a, b); }); }
};

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
