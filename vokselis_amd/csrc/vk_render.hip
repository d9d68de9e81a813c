// vk_render.hip -- vk_render / vk_render_partition: one raycast pass into the backbuffer (the reference's
// RaycastPipeline::record, examples/bonsai/raycast.rs / examples/xor/raycast.rs) -- argument checks, LaunchDesc, kernel choice.
#include "vk_ctx.hpp"
#include "vk_launch.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace vk;

// Argument and state checks shared by every render entry point; `cam` is the 144-byte camera the frame uses.
// The kernels' policy switches (vk_common.hpp: LaunchFlag) from the caller's VK_RENDER_* flags and the context's knobs.
uint32_t launch_flags(const vk_ctx *ctx, uint32_t render_flags, bool batch) {
    uint32_t f = 0;
    if (render_flags & VK_RENDER_DEBUG_TRIPS) f |= LF_STEPS_ARE_TRIPS;
    if (render_flags & VK_RENDER_DEBUG_FALLBACK) f |= LF_STEPS_ARE_FALLBACKS;
    if (!(render_flags & VK_RENDER_PROBE_ALWAYS)) f |= LF_ADAPTIVE_PROBING;
    if (ctx->wave_prio) f |= LF_WAVE_PRIORITY;
    if (ctx->setup_generic) f |= LF_SETUP_GENERIC;
    if (batch && ctx->frame_runs) f |= LF_FRAME_RUNS;
    // probe ahead pays where a frame's waves run against their own dependent chains -- a lone single-frame launch (-11 %) -- and costs where the
    // machine is full (+6-8 % in batches).  A frame of a ring in which three frames execute at once (k = 4) is in the second case: C2 0.0768 ->
    // 0.0724 ms per frame with the leaner kernel there, 0.080 -> 0.088 at k = 3 where two execute (profiles/r06_frames_in_flight.txt)
    const bool crowded = frames_crowded(ctx);
    if (ctx->probe_ahead == 1u || (ctx->probe_ahead == 2u && !batch && !crowded)) f |= LF_PROBE_AHEAD;  // (dispatch_march drops it for dt_scale > 1.25)
    return f;
}

int check_render(vk_ctx *ctx, int mode, const float *cam, float dt_scale, uint32_t ts, uint32_t rank, uint32_t nranks) {
    if (!ctx) return VK_ERR_INVALID;
    if (mode != VK_MODE_NAIVE_TRILINEAR && mode != VK_MODE_COMPUTE_NEAREST && mode != VK_MODE_PROCEDURAL) return fail(ctx, VK_ERR_INVALID, "unknown mode");
    if (ctx->format < 0 && mode != VK_MODE_PROCEDURAL) return fail(ctx, VK_ERR_INVALID, "render: no volume uploaded");
    if (!ctx->backbuffer) return fail(ctx, VK_ERR_INVALID, "render: no backbuffer (vk_backbuffer_resize)");
    if (!cam) return fail(ctx, VK_ERR_INVALID, "render: no camera (vk_set_camera)");
    // PROCEDURAL shares the compute twin's ray, box and step: geometry helpers treat it as that mode
    const int geo_mode = mode == VK_MODE_PROCEDURAL ? VK_MODE_COMPUTE_NEAREST : mode;
    if (mode == VK_MODE_NAIVE_TRILINEAR && ctx->format == VK_FMT_RGBA16F_PAIR)
        return fail(ctx, VK_ERR_INVALID, "NAIVE_TRILINEAR needs a scalar volume (R8_UNORM / R16_FLOAT / R16_UNORM)");
    if (mode == VK_MODE_COMPUTE_NEAREST && ctx->format != VK_FMT_RGBA16F_PAIR)
        return fail(ctx, VK_ERR_INVALID, "COMPUTE_NEAREST needs an RGBA16F_PAIR volume");
    if (!(dt_scale > 0.0f) || !std::isfinite(dt_scale)) return fail(ctx, VK_ERR_INVALID, "dt_scale must be finite and > 0");
    if (ts == 0 || (ts & 7u) || ts > 1024) return fail(ctx, VK_ERR_INVALID, "tile size must be a multiple of 8 in [8, 1024]");
    if (nranks == 0 || rank >= nranks) return fail(ctx, VK_ERR_INVALID, "rank/nranks");
    // Loop-termination guard (the reference would hang the GPU on a dt that no longer advances t):
    // t <= |eye - box| + box diagonal; require dt >= 8 ulp(t_max).
    {
        const float *e = cam;
        float reach = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + 4.0f;
        if (geo_mode == VK_MODE_COMPUTE_NEAREST) reach += 200.0f;  // near-plane point of a far=100 frustum
        float nmax = (float)std::max(ctx->nx, std::max(ctx->ny, ctx->nz));
        float dt_min = mode == VK_MODE_NAIVE_TRILINEAR ? dt_scale / nmax : dt_scale * 0.01f;
        float ulp = std::nextafter(reach, 2.0f * reach) - reach;
        if (!(dt_min >= 8.0f * ulp)) return fail(ctx, VK_ERR_UNSUPPORTED, "dt too small against the camera distance: the march would not advance");
    }
    return VK_OK;
}

// Launch the march kernel of the context's volume for a filled LaunchDesc (one frame or a batch).
// `reach_cam`: the camera whose distance decides whether the unclamped fast path is safe (the farthest of a batch).
// `geom`: the geometry pass of the isosurface (vk_render_geometry) -- every choice below is the colour render's, but for the kernel family.
int dispatch_march(vk_ctx *ctx, int mode, const LaunchDesc &L_in, uint32_t flags, const float *reach_cam, const GeomDesc *geom) {
    LaunchDesc L = L_in;
    // probe-ahead requests the distance byte of a position one step past a ray's end: inside the index tables' padding only while a step is
    // at most ~1.5 cells (vk_march.hpp: locate)
    if (!(L.dt_scale <= 1.25f)) L.flags &= ~(uint32_t)LF_PROBE_AHEAD;
    const bool count = (flags & VK_RENDER_COUNT) != 0;
    VolumeDesc V = volume_desc(ctx);  // (V.lut: the no-skip variants take the byte-offset copy, set where the variant is chosen)
    const uint64_t n_blocks = L.n_blocks;
    uint32_t grid = (uint32_t)((n_blocks + 511) / 512 * 512);
    L.grid_march = grid;
    // the block map's reciprocals (vk_hostmath.hpp): exact for every block index below n_blocks, or the launch is refused
    if (!block_map_make(L.ts, L.tiles_x, L.tiles_y, L.frames ? L.n_frames : 1u, L.nranks, L.root_skip, n_blocks, L.bm))
        return fail(ctx, VK_ERR_UNSUPPORTED, "launch too large for the block map: a smaller image, larger tiles or fewer frames per batch");
    // ... and the reciprocals of the image size for the rays' NDC coordinates
    L.rcp_w = 1.0f / (float)L.W;
    L.rcp_h = 1.0f / (float)L.H;
    // a runtime transfer function (vk_set_transfer_function) has kernels on the LINEAR / PACKED / PACKED_PAIRS layouts, walking with the loop
    // a first-hit isosurface (vk_set_isosurface): kernels of its own with the table kernels' coverage; table and projection are ignored under it, lighting is honoured
    const bool iso = mode == VK_MODE_NAIVE_TRILINEAR && ctx->iso_on;
    if (geom && !iso) return fail(ctx, VK_ERR_INVALID, "vk_render_geometry: no isosurface set (vk_set_isosurface)");
    const bool tf = mode == VK_MODE_NAIVE_TRILINEAR && ctx->d_tf && !iso;
    // the maximum-intensity projection (vk_set_projection): kernels of its own with the table kernels' coverage; lighting is ignored under it
    const bool mip = mode == VK_MODE_NAIVE_TRILINEAR && ctx->proj == VK_PROJ_MAX && !iso;
    // gradient lighting (vk_set_lighting) shades the table's colour: it has no kernels without a table
    if (mode == VK_MODE_NAIVE_TRILINEAR && ctx->lit && !tf && !mip && !iso)
        return fail(ctx, VK_ERR_UNSUPPORTED, "lighting: NAIVE_TRILINEAR renders with lighting need a transfer function (set a table with vk_set_transfer_function, or turn lighting off with vk_set_lighting(NULL))");
    // a clip box (vk_set_clip_box) is an argument of the table, lit, MAX and isosurface kernels: the built-in family has none
    if (mode == VK_MODE_NAIVE_TRILINEAR && ctx->clip_on && !tf && !mip && !iso)
        return fail(ctx, VK_ERR_UNSUPPORTED, "clip box: NAIVE_TRILINEAR renders under a clip box need a transfer function, VK_PROJ_MAX or an isosurface (the built-in march has no clip kernels; vk_set_clip_box(NULL) resets)");
    ClipDesc Cb{};
    for (int i = 0; i < 3; i++) { Cb.lo[i] = ctx->clip_lo[i]; Cb.hi[i] = ctx->clip_hi[i]; }
    const ClipDesc *Cl = mode == VK_MODE_NAIVE_TRILINEAR && ctx->clip_on ? &Cb : nullptr;  // nullptr: the kernels without a box
    IsoDesc I{};
    if (iso) {
        if (!has_table_layout(ctx->vol_kind))
            return fail(ctx, VK_ERR_UNSUPPORTED, "isosurface: NAIVE_TRILINEAR renders under an isosurface need a LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED have no isosurface kernels; vk_set_isosurface(NULL) resets)");
        if (flags & VK_RENDER_FAST_WALK) return fail(ctx, VK_ERR_UNSUPPORTED, "isosurface: VK_RENDER_FAST_WALK has no isosurface kernels");
        const char *bad = iso_desc(ctx->iso.iso, ctx->iso.rgb, ctx->iso.refine, format_scale(ctx->format), I);
        if (bad) return fail(ctx, VK_ERR_INVALID, std::string("isosurface: ") + bad);  // (vk_set_isosurface has checked it)
        I.lit = ctx->lit ? 1 : 0;
        I.light = ctx->light;
    }
    // light-direction shadows (vk_set_shadows) take effect under a lit isosurface whose light is not a headlight (a headlight's shadow ray runs back
    // along the primary ray, which was empty up to the hit): kernels of their own; in every other case the state is ignored
    const bool shadow = !geom && iso && ctx->shadows_on && ctx->lit && !ctx->light.headlight;
    ShadowDesc Sh{};
    if (shadow) {
        const char *bad = shadow_desc(ctx->shadows.strength, ctx->shadows.bias, Sh);
        if (bad) return fail(ctx, VK_ERR_INVALID, std::string("shadows: ") + bad);  // (vk_set_shadows has checked it)
    }
    TfDesc T{};
    if (mip || tf) {
        if (!has_table_layout(ctx->vol_kind))
            return fail(ctx, VK_ERR_UNSUPPORTED, mip ? "projection: NAIVE_TRILINEAR renders under VK_PROJ_MAX need a LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED have no maximum-projection kernels; vk_set_projection(VK_PROJ_COMPOSITE) resets)"
                                                     : "transfer function: NAIVE_TRILINEAR renders with a table need a LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED have no table kernels; vk_set_transfer_function(NULL) resets)");
        if (flags & VK_RENDER_FAST_WALK)
            return fail(ctx, VK_ERR_UNSUPPORTED, mip ? "projection: VK_RENDER_FAST_WALK has no maximum-projection kernels (VK_PROJ_MAX)" : "transfer function: VK_RENDER_FAST_WALK has no table kernels");
        // the window of the table in force; under VK_PROJ_MAX without one the implicit grey ramp, two entries over [0, 1] (T.rgba stays NULL)
        const uint32_t n = tf ? ctx->tf_n : 2u;
        tf_constants(n, tf ? ctx->tf_lo : 0.0f, tf ? ctx->tf_hi : 1.0f, format_scale(ctx->format), T.k1, T.k2);
        T.rgba = tf ? ctx->d_tf : nullptr;
        T.umax = (float)(n - 1u);
        T.imax = (int32_t)n - 2;
    }
    if (mode != VK_MODE_NAIVE_TRILINEAR) L.clear_max_inactive = 0;  // (their kernels have no clearing blocks: every tile is active)
    // whole-frame batches: the strips that clear the inactive tiles ride behind the march blocks (clear_inactive_strip)
    const uint64_t clear_blocks = (uint64_t)L.clear_max_inactive * L.n_frames * ((L.ts * L.ts + 511u) / 512u);
    if ((uint64_t)grid + clear_blocks >= (1ull << 31)) return fail(ctx, VK_ERR_UNSUPPORTED, "launch too large: fewer frames per batch");
    grid += (uint32_t)clear_blocks;
    if (grid == 0) return VK_OK;
    if (mode == VK_MODE_PROCEDURAL) {
        float time = 0.0f;
        std::memcpy(&time, ctx->uniform + 36, sizeof(float));  // Uniform.time (global_ubo.rs:52-65), what xor.wgsl reads as un.time
        if (!std::isfinite(time)) return fail(ctx, VK_ERR_INVALID, "Uniform.time must be finite");
        if ((flags & VK_RENDER_DEVICE_SINE) && count) return fail(ctx, VK_ERR_INVALID, "VK_RENDER_DEVICE_SINE is a tolerance mode: count steps with the specified sine");
        launch_procedural(ctx, L, grid, count, time, (flags & VK_RENDER_DEVICE_SINE) != 0);
    } else if (mode == VK_MODE_COMPUTE_NEAREST) {
        launch_compute(ctx, L, V, grid, count, ctx->vol_kind == VOL_PAIRB, !(flags & VK_RENDER_NO_SKIP));  // bricked 16-byte records, or the two dense volumes (the literal twin)
    } else {
        // Skipping costs a distance lookup per probing trip; it only pays when there is something to skip
        // (docs/archive/tools/skip_crossover.py, DESIGN.md section 4: on 256^3 volumes with a share e of exactly-transparent cells
        // the skip kernel overtakes the dense one between e = 0.36 and e = 0.56: 0.335 / 0.348 / 0.407 ms for dense /
        // adaptive / probing always at e = 0.36, 0.332 / 0.302 / 0.292 at e = 0.56).  Default policy by the census taken
        // at upload:  e < 0.45: the dense kernel;  0.45 <= e < 0.55: the skip kernel with adaptive probing (dense
        // stretches where nothing is being skipped);  e >= 0.55: the skip kernel probing on every trip (emptier
        // volumes -- the bonsai stand-in is at 0.77 -- spend their time in the skip walks, and the stretches only cost).
        // VK_RENDER_FORCE_SKIP takes the skip kernel whatever the census, adaptive unless VK_RENDER_PROBE_ALWAYS.
        const bool forced = (flags & VK_RENDER_FORCE_SKIP) != 0;
        const bool skip = !(flags & VK_RENDER_NO_SKIP) && (forced || ctx->empty_fraction >= 0.45);
        if (skip && !forced && ctx->empty_fraction >= 0.55) L.flags &= ~(uint32_t)LF_ADAPTIVE_PROBING;
        if (skip && ctx->empty_fraction < 0.05) L.flags |= LF_LONG_STRETCHES;  // forced on (almost) solid material: long dense stretches from the start
        // SAFE=false (no per-axis clamps, 32-bit offsets, index tables in LDS) only where cell_march_fast (vk_hostmath.hpp, with the
        // derivation) allows it: the cell array is < 4 GiB, the tables fit their LDS budget, and the camera's distance AND the length of the
        // longest ray (nmax / dt_scale trips: the f32 loop drifts by half an ulp of t and of p per trip, and runs on while its t says so)
        // keep every looked-up index inside the tables.  Frames are the same bits either way; vk_debug_march_path asks the same function.
        static_assert(kRenderSafeFlag == (uint32_t)VK_RENDER_SAFE, "vk_hostmath.hpp restates VK_RENDER_SAFE");
        const bool safe = !cell_march_fast(V.max_off, ctx->nx, ctx->ny, ctx->nz, reach_cam, L.dt_scale, flags);
        if (ctx->vol_kind == VOL_S8U8 || ctx->vol_kind == VOL_S8F16) launch_staged(ctx, L, V, grid, count, reach_cam);
        else if (is_u16_kind(ctx->vol_kind)) {  // an R16_UNORM volume: the same families, kernels of their own units (vk_march_u16.hpp)
            if (flags & VK_RENDER_FAST_WALK) return fail(ctx, VK_ERR_UNSUPPORTED, "R16_UNORM: VK_RENDER_FAST_WALK has no u16 kernels (the walks take the loop)");
            if (geom) launch_u16_geom(ctx, L, V, I, *geom, Cl, grid, skip, safe);
            else if (shadow) launch_u16_iso_shadow(ctx, L, V, I, Sh, Cl, grid, count, skip, safe);
            else if (iso) launch_u16_iso(ctx, L, V, T, ctx->light, I, Cl, grid, count, skip, safe);
            else if (mip) launch_u16_mip(ctx, L, V, T, ctx->light, I, Cl, grid, count, skip, safe);
            else if (tf && ctx->lit) launch_u16_lit(ctx, L, V, T, ctx->light, I, Cl, grid, count, skip, safe);
            else if (tf) launch_u16_tf(ctx, L, V, T, ctx->light, I, Cl, grid, count, skip, safe);
            else launch_u16_cells(ctx, L, V, T, ctx->light, I, nullptr, grid, count, skip, safe);
        }
        else if (geom) launch_cells_geom(ctx, L, V, I, *geom, Cl, grid, skip, safe);
        else if (shadow) launch_cells_iso_shadow(ctx, L, V, I, Sh, Cl, grid, count, skip, safe);
        else if (iso) launch_cells_iso(ctx, L, V, I, Cl, grid, count, skip, safe);
        else if (mip) launch_cells_mip(ctx, L, V, T, Cl, grid, count, skip, safe);
        else if (tf && ctx->lit) launch_cells_lit(ctx, L, V, T, ctx->light, Cl, grid, count, skip, safe);
        else if (tf) launch_cells_tf(ctx, L, V, T, Cl, grid, count, skip, safe);
        else launch_cells(ctx, L, V, grid, count, skip, safe, (flags & VK_RENDER_FAST_WALK) ? 2 : 0);  // (vk_march.hpp: WalkKind)
    }
    HIP_TRY(ctx, hipGetLastError());
    return VK_OK;
}

static int render_common(vk_ctx *ctx, int mode, int32_t ox, int32_t oy, uint32_t rw, uint32_t rh, uint32_t ts,
                         uint32_t rank, uint32_t nranks, float dt_scale, uint32_t flags, void *compact_out, const GeomDesc *geom = nullptr) {
    if (!ctx) return VK_ERR_INVALID;
    int crc = check_render(ctx, mode, ctx->have_camera ? ctx->camera : nullptr, dt_scale, ts, rank, nranks);
    if (crc) return crc;
    const int geo_mode = mode == VK_MODE_PROCEDURAL ? VK_MODE_COMPUTE_NEAREST : mode;
    constexpr uint32_t kPresentFlags = VK_RENDER_PRESENT | VK_RENDER_PRESENT_BGRA | VK_RENDER_PRESENT_ONLY;
    if ((flags & kPresentFlags) && compact_out) return fail(ctx, VK_ERR_INVALID, "VK_RENDER_PRESENT*: whole-pixel passes into the backbuffer only (vk_render)");
    if (rw == 0 || rh == 0) return VK_OK;  // empty tile
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (flags & kPresentFlags) {  // the present target at the backbuffer's own size, as vk_present(width, height) would make it
        int prc = present_targets(ctx, ctx->width, ctx->height, (flags & VK_RENDER_PRESENT_BGRA) != 0);
        if (prc) return prc;
    }
    const bool count = (flags & VK_RENDER_COUNT) != 0;
    if (count && !ctx->steps) {
        if (hipError_t ae = ctx_alloc(ctx, (void **)&ctx->steps, (size_t)ctx->width * ctx->height * sizeof(uint32_t))) return alloc_failed(ctx, ae, "render", "the step image");
        HIP_TRY(ctx, hipMemsetAsync(ctx->steps, 0, (size_t)ctx->width * ctx->height * sizeof(uint32_t), ctx->stream));
    }
    LaunchDesc L{};
    L.eye[0] = ctx->camera[0]; L.eye[1] = ctx->camera[1]; L.eye[2] = ctx->camera[2]; L.eye[3] = ctx->camera[3];
    std::memcpy(L.inv_proj, ctx->camera + 20, 64);
    L.W = ctx->width; L.H = ctx->height;
    L.ox = ox; L.oy = oy; L.rw = rw; L.rh = rh;
    L.ts = ts;
    L.tiles_x = (rw + ts - 1) / ts;
    L.tiles_y = (rh + ts - 1) / ts;
    {
        int32_t cr[4];
        cull_rect_cam(ctx, ctx->camera, geo_mode, cr);
        L.cull_x0 = cr[0]; L.cull_y0 = cr[1]; L.cull_x1 = cr[2]; L.cull_y1 = cr[3];
    }
    L.rank = rank; L.nranks = nranks;
    // whole-pixel launches of few tiles (C2 at 64-pixel tiles: 510) carry the order in their arguments; partitions and large tile counts
    // read the device table (the partition's un-tile needs it there anyway)
    const bool order_inline = !compact_out && (uint64_t)L.tiles_x * L.tiles_y <= kOrderInline && !ctx->order_never_inline;
    {
        int orc = tile_order_update(ctx, geo_mode, ox, oy, rw, rh, ts, !order_inline);
        if (orc) return orc;
        if (order_inline) {
            for (size_t q = 0; q < ctx->order.size(); q++) L.order_inline[q] = (uint16_t)ctx->order[q];
            L.tile_order = nullptr;
        } else {
            orc = order_wait(ctx);
            if (orc) return orc;
            L.tile_order = ctx->d_order;
        }
    }
    // a partition (compact output) covers only the active tiles; a plain render covers the whole region
    const uint64_t tiles = compact_out ? (uint64_t)ctx->order_active : (uint64_t)L.tiles_x * L.tiles_y;
    L.root_skip = nranks > 1 ? ctx->root_skip : 0u;
    const uint64_t slots = deal_rounds((uint32_t)tiles, nranks, L.root_skip);
    L.n_tiles_launch = (uint32_t)tiles;
    // (PROCEDURAL / COMPUTE_NEAREST: every tile is active; the naive and staged kernels are the ones that test it)
    L.n_active_tiles = ctx->order_active;
    if (tiles == 0) return VK_OK;
    const uint64_t per_tile = (uint64_t)(ts / 8) * (ts / 8);
    const uint64_t n_blocks = slots * per_tile;
    if (n_blocks >= (1ull << 31) - 512) return fail(ctx, VK_ERR_UNSUPPORTED, "launch too large");
    L.n_blocks = (uint32_t)n_blocks;
    L.compact = compact_out ? 1u + (uint32_t)ctx->wire : 0u;
    L.dt_scale = dt_scale;
    L.out = compact_out ? compact_out : ctx->backbuffer;
    L.steps = count ? ctx->steps : nullptr;
    L.counters = count ? ctx->counters : nullptr;
    L.trace = nullptr;
    L.frames = nullptr;
    L.n_frames = 1;
    L.flags = launch_flags(ctx, flags, false) | (order_inline ? (uint32_t)LF_ORDER_INLINE : 0u);
    L.walk_cap = ctx->walk_cap ? (float)ctx->walk_cap : HUGE_VALF;
    L.walk_cap_all = ctx->walk_cap_all ? (float)ctx->walk_cap_all : HUGE_VALF;
    L.pair_walk_min = ctx->pair_walk_min;
    if (flags & kPresentFlags) {
        L.present_rgba8 = ctx->rgba8;
        L.present_bgra8 = (flags & VK_RENDER_PRESENT_BGRA) ? ctx->bgra8 : nullptr;
        L.present_only = (flags & VK_RENDER_PRESENT_ONLY) ? 1u : 0u;
    }
    if (count && ctx->want_trace) {
        // (a per-trip log of trip_log_cap u32 per wave = trip_log_cap / 8 records of the stamps' size)
        const uint64_t recs = ctx->trip_log_cap ? n_blocks * (ctx->trip_log_cap / 8u) : n_blocks;
        if (ctx->trace_blocks < recs) {
            if (ctx->trace) (void)hipFree(ctx->trace);
            ctx->trace = nullptr; ctx->trace_blocks = 0;
            if (hipError_t ae = ctx_alloc(ctx, (void **)&ctx->trace, recs * 4 * sizeof(unsigned long long))) return alloc_failed(ctx, ae, "render", "the wave trace");
            ctx->trace_blocks = recs;
        }
        // start = +inf (atomicMin), end = 0 (atomicMax): fill {0xff.., 0} pairs
        std::vector<unsigned long long> init(recs * 4, 0ull);
        if (ctx->trip_log_cap) { L.flags |= LF_TRIP_LOG; L.trip_log_cap = ctx->trip_log_cap; }
        else for (uint64_t i = 0; i < n_blocks; i++) init[4 * i] = ~0ull;
        HIP_TRY(ctx, hipMemcpy(ctx->trace, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
        L.trace = ctx->trace;
    }
    return dispatch_march(ctx, mode, L, flags, ctx->camera, geom);
}

// Fill of a freshly allocated geometry surface with the miss record (the record is not one repeated byte): one thread per pixel.
__global__ __launch_bounds__(256) void geom_fill_kernel(float4 *surface, size_t n_pixels) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_pixels) return;
    surface[2 * i] = geom_miss0();
    surface[2 * i + 1] = geom_miss1();
}

extern "C" {

// Lighting is host state read by dispatch_march when a render is recorded: nothing on the device changes, so no drain, no map rebuild, and no
// restriction to the outside of vk_frame_begin / vk_frame_end.
int vk_set_lighting(vk_ctx *ctx, const vk_lighting *light) {
    if (!ctx) return VK_ERR_INVALID;
    if (!light) {
        ctx->lit = false;
        return VK_OK;
    }
    LightDesc D{};
    if (const char *why = light_desc(light->dir, light->headlight, light->ambient, light->diffuse, light->specular, light->shininess, D))
        return fail(ctx, VK_ERR_INVALID, std::string("vk_set_lighting: ") + why);
    ctx->light = D;
    ctx->lit = true;
    return VK_OK;
}

// Shadows are host state like lighting, read by dispatch_march when a render is recorded: no drain, no map rebuild (the skip maps are the
// isosurface's), settable inside a frame; they stay in force across uploads.
int vk_set_shadows(vk_ctx *ctx, const vk_shadows *s) {
    if (!ctx) return VK_ERR_INVALID;
    if (!s) {
        ctx->shadows_on = false;
        return VK_OK;
    }
    ShadowDesc D{};
    if (const char *why = shadow_desc(s->strength, s->bias, D)) return fail(ctx, VK_ERR_INVALID, std::string("vk_set_shadows: ") + why);
    ctx->shadows.strength = s->strength + 0.0f;
    ctx->shadows.bias = D.bias;
    ctx->shadows_on = true;
    return VK_OK;
}

int vk_get_shadows(vk_ctx *ctx, vk_shadows *out, int *enabled) {
    if (!ctx) return VK_ERR_INVALID;
    if (enabled) *enabled = ctx->shadows_on ? 1 : 0;
    if (out && ctx->shadows_on) *out = ctx->shadows;
    return VK_OK;
}

// The clip box is host state like lighting: dispatch_march takes it into the kernel arguments and vk_order.hip into the frame's screen-space
// geometry when a render is recorded.  No drain, no map rebuild; the cached tile orders carry it in their keys.
int vk_set_clip_box(vk_ctx *ctx, const vk_clip_box *box) {
    if (!ctx) return VK_ERR_INVALID;
    if (!box) {
        ctx->clip_on = false;
        return VK_OK;
    }
    for (int i = 0; i < 3; i++) {
        if (!std::isfinite(box->lo[i]) || !std::isfinite(box->hi[i])) return fail(ctx, VK_ERR_INVALID, "vk_set_clip_box: a component is not finite");
        if (!(0.0f <= box->lo[i] && box->lo[i] < box->hi[i] && box->hi[i] <= 1.0f))
            return fail(ctx, VK_ERR_INVALID, "vk_set_clip_box: needs 0 <= lo < hi <= 1 on every axis");
    }
    for (int i = 0; i < 3; i++) { ctx->clip_lo[i] = box->lo[i] + 0.0f; ctx->clip_hi[i] = box->hi[i]; }  // (+ 0: a -0 bound is stored as +0)
    ctx->clip_on = true;
    return VK_OK;
}

int vk_get_clip_box(vk_ctx *ctx, vk_clip_box *out, int *enabled) {
    if (!ctx) return VK_ERR_INVALID;
    if (enabled) *enabled = ctx->clip_on ? 1 : 0;
    if (out && ctx->clip_on)
        for (int i = 0; i < 3; i++) { out->lo[i] = ctx->clip_lo[i]; out->hi[i] = ctx->clip_hi[i]; }
    return VK_OK;
}

int vk_render(vk_ctx *ctx, int mode, int32_t tile_x, int32_t tile_y, uint32_t tile_w, uint32_t tile_h, float dt_scale,
              uint32_t flags) {
    // tiles of the launch order: 64 x 64 pixels; 32 x 32 for the staged march, whose waves are few and long (C4 1.80 -> 1.68 ms, C5 9.40 -> 9.02;
    // C2 and the compute twin lose 0.5 - 4 % at 32)
    const bool staged = ctx && (ctx->vol_kind == vk::VOL_S8U8 || ctx->vol_kind == vk::VOL_S8F16) && mode == VK_MODE_NAIVE_TRILINEAR;
    return render_common(ctx, mode, tile_x, tile_y, tile_w, tile_h, ctx && ctx->render_tile ? ctx->render_tile : (staged ? 32u : 64u), 0, 1, dt_scale, flags, nullptr);
}

// The geometry pass of the first-hit isosurface: render_common's launch -- cull rectangle, active tiles, tile order,
// fast-path condition and policy flags are the colour render's by construction -- with the geometry kernels, into the current slot's
// geometry surface.  The surface is allocated, and filled with the miss record, by the slot's first pass since the last resize.
int vk_render_geometry(vk_ctx *ctx, int32_t tile_x, int32_t tile_y, uint32_t tile_w, uint32_t tile_h, float dt_scale, uint32_t flags) {
    if (!ctx) return VK_ERR_INVALID;
    bool unsupported = false;
    if (const char *why = geom_flags_check(flags, &unsupported)) return fail(ctx, unsupported ? VK_ERR_UNSUPPORTED : VK_ERR_INVALID, why);
    const uint32_t ts = ctx->render_tile ? ctx->render_tile : 64u;
    int crc = check_render(ctx, VK_MODE_NAIVE_TRILINEAR, ctx->have_camera ? ctx->camera : nullptr, dt_scale, ts, 0, 1);
    if (crc) return crc;
    if (!ctx->iso_on) return fail(ctx, VK_ERR_INVALID, "vk_render_geometry: no isosurface set (vk_set_isosurface)");
    if (!has_table_layout(ctx->vol_kind))
        return fail(ctx, VK_ERR_UNSUPPORTED, "isosurface: the geometry pass needs a LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED have no isosurface kernels)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->geom) {
        const size_t n = (size_t)ctx->width * ctx->height;
        if (hipError_t ae = ctx_alloc(ctx, &ctx->geom, geom_surface_bytes(ctx->width, ctx->height))) return alloc_failed(ctx, ae, "vk_render_geometry", "the geometry surface");
        hipLaunchKernelGGL(geom_fill_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, ctx->stream, reinterpret_cast<float4 *>(ctx->geom), n);
        HIP_TRY(ctx, hipGetLastError());
    }
    GeomDesc G{};
    G.surface = ctx->geom;
    return render_common(ctx, VK_MODE_NAIVE_TRILINEAR, tile_x, tile_y, tile_w, tile_h, ts, 0, 1, dt_scale, flags, nullptr, &G);
}

// One pixel's record: the 1 x 1 tile at (x, y) into the current slot's surface, then that record.  The ray does not depend on the tile,
// so the record is the full-frame pass's, bit for bit.
int vk_pick(vk_ctx *ctx, uint32_t x, uint32_t y, float dt_scale, vk_hit *out) {
    if (!ctx) return VK_ERR_INVALID;
    if (!out) return fail(ctx, VK_ERR_INVALID, "vk_pick: out is NULL");
    if (!ctx->backbuffer) return fail(ctx, VK_ERR_INVALID, "render: no backbuffer (vk_backbuffer_resize)");
    if (x >= ctx->width || y >= ctx->height) return fail(ctx, VK_ERR_INVALID, "vk_pick: the pixel lies outside the backbuffer");
    int rc = vk_render_geometry(ctx, (int32_t)x, (int32_t)y, 1, 1, dt_scale, 0);
    if (rc) return rc;
    float rec[8];
    HIP_TRY(ctx, hipMemcpyAsync(rec, reinterpret_cast<const char *>(ctx->geom) + geom_record_offset(x, y, geom_row_bytes(ctx->width)), sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    out->hit = std::isfinite(rec[3]) ? 1 : 0;
    for (int i = 0; i < 3; i++) { out->pos[i] = rec[i]; out->grad[i] = rec[4 + i]; }
    out->t = rec[3];
    out->value = rec[7];
    return VK_OK;
}

// The slice pass: a kernel family of its own (vk_launch_slice.hip), no camera, no tile order, no cull.  The plane comes
// with the call; table, clip box and format are the context's.  Every refusal comes before the first write: the backbuffer is untouched.
int vk_render_slice(vk_ctx *ctx, const vk_slice *slice, int32_t tile_x, int32_t tile_y, uint32_t tile_w, uint32_t tile_h, uint32_t flags) {
    if (!ctx) return VK_ERR_INVALID;
    if (flags & ~(uint32_t)VK_SLICE_VALUES) return fail(ctx, VK_ERR_INVALID, "vk_render_slice: takes VK_SLICE_VALUES only");
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, "vk_render_slice", "slice")) return rc;
    if (!ctx->backbuffer) return fail(ctx, VK_ERR_INVALID, "vk_render_slice: no backbuffer (vk_backbuffer_resize)");
    SliceDesc S{};
    const bool tf = ctx->d_tf != nullptr;
    if (const char *why = slice_validate(slice, tf ? ctx->tf_n : 0u, ctx->tf_lo, ctx->tf_hi, format_scale(ctx->format), S))
        return fail(ctx, VK_ERR_INVALID, std::string("vk_render_slice: ") + why);
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, "vk_render_slice", "slice", "slice pass")) return rc;
    if (!slice_tile_clip(tile_x, tile_y, tile_w, tile_h, ctx->width, ctx->height, S.x0, S.y0, S.x1, S.y1)) return VK_OK;  // no pixel of the tile on the backbuffer
    if ((S.y1 - S.y0 + 7u) / 8u > 65535u) return fail(ctx, VK_ERR_UNSUPPORTED, "slice: tile too tall for one launch");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if ((flags & VK_SLICE_VALUES) && !ctx->slice_values) {
        if (hipError_t ae = ctx_alloc(ctx, &ctx->slice_values, slice_surface_bytes(ctx->width, ctx->height))) return alloc_failed(ctx, ae, "vk_render_slice", "the value surface");
        HIP_TRY(ctx, hipMemsetAsync(ctx->slice_values, 0, slice_surface_bytes(ctx->width, ctx->height), ctx->stream));
    }
    for (int i = 0; i < 3; i++) { S.lo[i] = ctx->clip_on ? ctx->clip_lo[i] : 0.0f; S.hi[i] = ctx->clip_on ? ctx->clip_hi[i] : 1.0f; }
    S.rgba = tf ? ctx->d_tf : nullptr;
    S.out = ctx->backbuffer;
    S.values = (flags & VK_SLICE_VALUES) ? ctx->slice_values : nullptr;
    S.W = ctx->width; S.H = ctx->height;
    launch_slice(ctx, volume_desc(ctx), S);
    HIP_TRY(ctx, hipGetLastError());
    return VK_OK;
}

// One pixel's sample: the 1 x 1 tile at (x, y) with VK_SLICE_VALUES into the current slot's surfaces, then that record.  The position does
// not depend on the tile, so the record is the full-frame pass's, bit for bit; pos is slice_position() on the host, the kernel's function.
int vk_slice_probe(vk_ctx *ctx, const vk_slice *slice, uint32_t x, uint32_t y, vk_slice_sample *out) {
    if (!ctx) return VK_ERR_INVALID;
    if (!out) return fail(ctx, VK_ERR_INVALID, "vk_slice_probe: out is NULL");
    if (!ctx->backbuffer) return fail(ctx, VK_ERR_INVALID, "vk_render_slice: no backbuffer (vk_backbuffer_resize)");
    if (x >= ctx->width || y >= ctx->height) return fail(ctx, VK_ERR_INVALID, "vk_slice_probe: the pixel lies outside the backbuffer");
    int rc = vk_render_slice(ctx, slice, (int32_t)x, (int32_t)y, 1, 1, VK_SLICE_VALUES);
    if (rc) return rc;
    float rec[2];
    HIP_TRY(ctx, hipMemcpyAsync(rec, reinterpret_cast<const char *>(ctx->slice_values) + slice_record_offset(x, y, slice_row_bytes(ctx->width)), sizeof(rec), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    out->inside = rec[1] != 0.0f ? 1 : 0;
    for (int i = 0; i < 3; i++) out->pos[i] = slice_position(slice->origin[i], slice->du[i], slice->dv[i], x, y);
    out->value = rec[0];
    return VK_OK;
}

// Debug: the build vk_render(ctx, VK_MODE_NAIVE_TRILINEAR, ..., dt_scale, flags) would launch now -- dispatch_march's own question, asked
// of the same function.  0 on the layouts that are always clamped.
int vk_debug_march_path(vk_ctx *ctx, float dt_scale, uint32_t flags, int *fast) {
    if (!ctx) return VK_ERR_INVALID;
    if (!fast) return fail(ctx, VK_ERR_INVALID, "vk_debug_march_path: fast is NULL");
    if (ctx->format < 0) return fail(ctx, VK_ERR_INVALID, "vk_debug_march_path: no volume uploaded");
    if (!ctx->have_camera) return fail(ctx, VK_ERR_INVALID, "vk_debug_march_path: no camera (vk_set_camera)");
    if (!(dt_scale > 0.0f) || !std::isfinite(dt_scale)) return fail(ctx, VK_ERR_INVALID, "dt_scale must be finite and > 0");
    *fast = is_cell_layout(ctx->vol_kind) && cell_march_fast(volume_desc(ctx).max_off, ctx->nx, ctx->ny, ctx->nz, ctx->camera, dt_scale, flags) ? 1 : 0;
    return VK_OK;
}

int vk_render_partition(vk_ctx *ctx, int mode, uint32_t tile_size, uint32_t rank, uint32_t nranks, float dt_scale,
                        uint32_t flags, void *compact_out) {
    if (!ctx) return VK_ERR_INVALID;
    if (!compact_out) return fail(ctx, VK_ERR_INVALID, "vk_render_partition: compact_out is NULL");
    return render_common(ctx, mode, 0, 0, ctx->width, ctx->height, tile_size, rank, nranks, dt_scale, flags, compact_out);
}

}  // extern "C"
