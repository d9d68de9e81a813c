// vk_ctx.hpp -- the context behind the C-ABI (include/vokselis_hip.h) and what the library's translation units share.
// Internal: nothing here is part of the boundary.
//
//   vk_context.hip         context lifetime, uniforms, backbuffer, read-back, counters, timers, tuning knobs
//   vk_volume.hip          vk_volume_*: re-layout of the uploaded / generated volume (VolBuild, transactional commit)
//   vk_order.hip           screen-space cull, heaviest-first tile order, vk_partition_* / vk_tiles_active
//   vk_render.hip          vk_render / vk_render_partition: argument checks, LaunchDesc, kernel choice
//   vk_batch.hip           vk_render_batch: many frames, one launch
//   vk_launch_cells.hip    instantiates the cell-layout march kernels      (vk_march.hpp)
//   vk_launch_tf.hip       instantiates the cell march under a transfer table (vk_march.hpp)
//   vk_launch_lit.hip      instantiates the table march with gradient lighting (vk_march.hpp, vk_light.hpp)
//   vk_launch_mip.hip      instantiates the cell march under the maximum-intensity projection (vk_march.hpp, vk_march_mip.hpp)
//   vk_launch_iso.hip      instantiates the cell march under a first-hit isosurface (vk_march.hpp, vk_march_iso.hpp, vk_iso.hpp)
//   vk_launch_iso_shadow.hip  instantiates the isosurface march with light-direction shadows (vk_march_iso.hpp, vk_shadow.hpp)
//   vk_launch_geom.hip     instantiates the geometry pass of the isosurface march (vk_march_iso.hpp, vk_geom.hpp)
//   vk_launch_slice.hip    the slice pass: a plane through the volume, thick slabs (vk_slice.hpp)
//   vk_launch_hist.hip     vk_volume_histogram, vk_histogram_window: histogram and statistics of a voxel box (vk_hist.hpp)
//   vk_launch_mesh.hip     vk_extract_isosurface: the isosurface as a triangle mesh, count / scan / emit (vk_mesh.hpp)
//   vk_launch_filter.hip   vk_volume_filter, vk_filter_gaussian: separable convolution and 3x3x3 median of the volume (vk_filter.hpp)
//   vk_launch_label.hip    vk_label_components: connected components of a value range, keep or drop them (vk_label.hpp)
//   vk_launch_dist.hip     vk_distance_transform: exact Euclidean distance transform of a value range, morphology by a radius (vk_dist.hpp)
//   vk_launch_resample.hip vk_volume_resample: a voxel box of the volume into other dimensions and another scalar format (vk_resample.hpp)
//   vk_launch_staged.hip   instantiates the LDS-staged march kernels       (vk_staged.hpp)
//   vk_launch_compute.hip  instantiates the compute twin and C3            (vk_compute.hpp)
//   vk_post.hip            clear, un-tile, present, capture                (vk_post.hpp)
//   vk_comm.hip            RCCL: vk_comm_*, vk_gather_tiles, vk_group_*
#pragma once

#include "../../include/vokselis_hip.h"
#include "vk_alloc_hook.hpp"
#include "vk_common.hpp"
#include "vk_geom.hpp"
#include "vk_iso.hpp"
#include "vk_light.hpp"
#include "vk_shadow.hpp"
#include "vk_slice.hpp"
#include "vk_tf.hpp"

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is loaded on first use (vk_comm.hip)

#include <string>
#include <utility>
#include <vector>

constexpr size_t kCounters = 10;  // vk_ctx::counters

struct vk_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    hipDeviceProp_t prop{};
    vk::AllocFailHook alloc_fail;  // debug, tests: which of the context's next allocations fails (vk_debug_set_param "alloc_fail_at"; ctx_alloc below)

    // volume
    void *vol = nullptr, *vol2 = nullptr;  // cells / dense voxels / pair
    void *scopy[3] = {nullptr, nullptr, nullptr};  // VK_LAYOUT_STAGED: one brick copy per slow axis
    vk::StagedDesc sdesc{};
    uint32_t stage_cap_bytes = 0, stage_slab_cells = 0, stage_copies_mask = 7;  // tunables (vk_debug_set_param)
    uint32_t stage_group = 2;    // staged march: one LDS window per 256-thread group of four waves (vk_staged.hpp: raymarch_staged_group_kernel): 0 never, 1 always, 2 where it pays (launch_staged)
    uint32_t frame_runs = 1;     // batched launches: every XCD marches a run of consecutive frames of a tile position (0: frames x, x + 8, ... as in round 2)
    uint32_t stage_grow_every = 0;  // slab search: try one cell above the last fit every n-th round (0: 4 for u8, 1 for f16; docs/archive/tools/staged_grow.py)
    uint32_t stage_row_pad = 2;  // odd LDS row pitch of the staged window: 0 never, 1 always, 2 (default) with group windows on u8 volumes (launch_staged)
    uint8_t *dist = nullptr;
    uint32_t *lut = nullptr;  // per-axis cell-index tables (cell units | byte offsets), cell layouts only
    size_t vol_bytes = 0;
    uint32_t nx = 0, ny = 0, nz = 0, nbx = 0, nby = 0, nbz = 0;
    int format = -1, layout = 0;
    int vol_kind = -1;  // vk::VolKind
    double empty_fraction = 0.0;  // share of cells that are exactly transparent (packed layouts)
    vk::VolumeDesc vdesc{};
    // runtime transfer function (vk_set_transfer_function): d_tf holds the n RGBA entries, then the n + 1 prefix counts of non-zero
    // alphas the emptiness predicate reads (vk_tf.hpp); nullptr: the built-in transfer
    float *d_tf = nullptr;
    uint32_t tf_n = 0;
    float tf_lo = 0.0f, tf_hi = 1.0f;
    // projection of NAIVE_TRILINEAR (vk_set_projection): compositing, or the maximum over the table's window (vk_launch_mip.hip)
    int proj = VK_PROJ_COMPOSITE;
    // first-hit isosurface of NAIVE_TRILINEAR (vk_set_isosurface; vk_launch_iso.hip): while set, it replaces table and projection, which stay stored
    bool iso_on = false;
    vk_isosurface iso{};
    // gradient lighting of the table march (vk_set_lighting): host state, passed by value to the lit kernels
    bool lit = false;
    vk::LightDesc light{};
    // light-direction shadows of the lit isosurface (vk_set_shadows): host state like lighting, passed by value to the shadow kernels
    bool shadows_on = false;
    vk_shadows shadows{};
    // clip box of the table, lit, MAX and isosurface marches (vk_set_clip_box): host state like lighting, in unit-cube coordinates; it also
    // tightens the host's screen-space geometry (vk_order.hip) and is part of the cached orders' keys
    bool clip_on = false;
    float clip_lo[3] = {0.0f, 0.0f, 0.0f}, clip_hi[3] = {1.0f, 1.0f, 1.0f};

    // uniforms (host copies; passed to kernels by value)
    unsigned char uniform[48] = {0};
    float camera[36] = {0};  // 144-byte CameraUniform
    bool have_camera = false;

    // output
    void *backbuffer = nullptr;
    uint32_t width = 0, height = 0;
    int out_format = VK_OUT_RGBA32F;
    uint32_t *steps = nullptr;
    void *geom = nullptr;  // the geometry surface of the current slot (vk_render_geometry): [height][width][2] float4, allocated by the slot's first geometry pass
    void *slice_values = nullptr;  // the value surface of the current slot (vk_render_slice under VK_SLICE_VALUES): [height][width] records of two f32, allocated and zero-filled by the slot's first such pass
    unsigned long long *counters = nullptr;  // kCounters of them: 0-5 the march's steps and census, 7 the upload's empty cells, 8-9 the lone-speckle census

    // heaviest-first tile order (launch-order heuristic; see tile_order_update)
    std::vector<uint32_t> order, order_pos;
    uint32_t order_active = 0;  // leading positions of `order` whose tiles can contain non-clear pixels
    bool order_on_device = false;  // the current slot of the device ring holds `order` / `order_pos` (single-frame launches of few tiles carry the order in their kernel arguments)
    std::vector<unsigned char> order_key;
    unsigned long long *trace = nullptr;
    size_t trace_blocks = 0;
    int wire = VK_WIRE_RGBA;     // compact tiles of a partition: whole pixels, or colour only (vk_partition_wire)
    bool want_trace = false;
    uint32_t trip_log_cap = 0;   // > 0: the trace buffer holds per-trip logs of that many u32 entries per wave instead of stamps (docs/archive/tools/repack_census.py)
    // The device copies of (order, order_pos) live in a ring of kOrderRing slots fed from pinned staging: a new
    // camera takes the next slot with one stream-ordered copy -- no host or device synchronisation -- while
    // launches still in flight (other streams: frames in flight) keep reading the slots they were given.
    uint32_t *d_order = nullptr, *d_order_pos = nullptr;  // the current slot
    uint32_t *d_ring = nullptr, *h_ring = nullptr;
    size_t d_order_cap = 0;      // entries per table in every slot
    int ring_slot = -1;
    hipEvent_t ring_ev[16] = {};     // slot uploaded
    hipStream_t ring_stream[16] = {};
    bool ring_done[16] = {};
    uint32_t ring_active[16] = {};   // order_active of the slot
    uint32_t order_seq = 0;          // order changes so far; change e lives in slot e % 16
    hipStream_t ring_use_stream[16] = {};  // frames in flight: the stream of the slot's last reader ...
    uint64_t ring_use_frame[16] = {};      // ... and the frame it belonged to (0: launched outside vk_frame_begin / vk_frame_end)
    hipEvent_t ring_guard_ev = nullptr;

    // batched launches (vk_render_batch): per-batch tables {FrameDesc[B], order[B][n_tiles], pos[B][n_tiles]} in a small
    // ring of device slots fed from pinned staging; a slot is rewritten only after the last kernel that read it
    struct BatchSlot {
        unsigned char *d = nullptr, *h = nullptr;
        size_t cap = 0;
        hipEvent_t ev = nullptr;
        uint32_t id = 0, n_frames = 0, n_tiles = 0, ts = 0, nranks = 0, max_active = 0, root_skip = 0;
        uint32_t width = 0, height = 0;  // the frame shape and pixel format the batch was dealt for: an un-tile under another
        int out_format = -1;             // shape (vk_backbuffer_resize in between) would scatter tiles out of bounds
        int wire = 0;                    // ... and the wire format its compact tiles were written in
    } batch[4];
    uint32_t batch_seq = 0;
    // table blocks a growing batch has outgrown: hipFree / hipHostFree synchronise the device, so they wait here for a
    // call that synchronises anyway (vk_backbuffer_resize, vk_ctx_destroy) instead of stalling four launches in flight
    std::vector<std::pair<void *, void *>> batch_retired;
    // the order of the last camera a batch computed one for (a still camera costs no host work from batch to batch)
    std::vector<unsigned char> batch_key;
    std::vector<uint32_t> batch_order, batch_pos;
    uint32_t batch_n_active = 0;
    // Skip kernels: steps a walk may take in a trip in which other lanes sample / in which every lane walks (0: no cap).
    // docs/archive/tools/walk_cap_sweep.py: 8 / 12 -- C2 0.0806 -> 0.0728 ms per frame in batches, 0.1625 -> 0.1555 single; a fog with
    // 80 % of its 16^3 blocks knocked out 0.161 -> 0.135.  Multiples of the walk loop's four steps do best.
    uint32_t walk_cap = 8, walk_cap_all = 12;
    uint32_t render_tile = 0;    // vk_render: tile size of the launch order (0: 64, 32 for the staged march)
    uint32_t pair_ring = 0;      // compute twin: request buffers in the SHADE ring (4, 6; 42: 4 buffers, two revolutions per loop iteration; 0: by launch shape)
    uint32_t pair_walk_min = 4;  // compute twin: shortest run of empty records worth a walk (a walk restarts the request ring; docs/archive/tools/compute_mode.py)
    uint32_t probe_ahead = 2;    // skip kernels: request the next position's distance byte under the sample (0 never, 1 always, 2 single-frame launches)
    uint32_t speckle_codes = 1;  // the built-in skip maps carry lone-speckle codes (vk_tf.hpp); 0 (debug, next map build): plain distances, every such cell is sampled
    uint32_t order_rays = 3;     // estimate rays per tile edge of the heaviest-first order (single-frame launches)
    uint32_t order_rays_batch = 1;  // ... of launches spanning >= 4 frames
    uint32_t order_never_inline = 0;  // debug / A-B: single-frame launches read the tile order from the device table as before round 6
    uint32_t setup_generic = 0;  // debug / A-B: the cell march's ray set-up with the generic divisions in every wave (LF_SETUP_GENERIC)
    uint32_t wave_prio = 1;      // issue priority by ray length (set_wave_priority); 0 for A/B measurements
    uint32_t naive_lds_pad = 0;  // debug: extra dynamic LDS per workgroup of the cell kernels (caps the waves per SIMD)
    uint32_t root_skip = 0;  // dealing: rank 0 sits out every root_skip-th round (vk_partition_root_skip)
    uint32_t hist_max_blocks = 0;    // vk_volume_histogram: cap of the grid (0: none) -- lets a small volume drive the grid-stride loop
    uint32_t hist_flush_passes = 0;  // ... and passes of that loop between merges of a workgroup's counters (0: vk_hist.hpp's bound)
    uint32_t mesh_chunk_cubes = 0;   // vk_extract_isosurface: cubes per chunk of the scan (0: vk_mesh.hpp's 1024; 64 .. 4096) -- lets a small volume have many chunks
    uint32_t mesh_max_blocks = 0;    // ... and cap of the count and emit grids (0: none)
    uint32_t filter_max_blocks = 0;  // vk_volume_filter: cap of the grid (0: none) -- lets a small volume drive the grid-stride loop over tiles
    uint32_t filter_timing = 0;      // ... 1 (measurements): the call brackets its kernel with the timer's events, vk_timer_elapsed_ms then reads the kernel alone
    uint32_t label_max_blocks = 0;   // vk_label_components: cap of every grid (0: none) -- lets a small volume drive the grid-stride loops over tiles and chunks
    uint32_t label_timing = 0;       // ... k (measurements): the call brackets its k-th kernel with the timer's events (1 tile, 2 seam, 3 flatten, 4 scan, 5 number, 6 label, 7 mask)
    uint32_t dist_max_blocks = 0;    // vk_distance_transform: cap of every grid (0: none) -- lets a small volume drive the grid-stride loops over columns, lines and voxels
    uint32_t dist_x_plain = 0;       // ... 1 (measurements, tests): the x pass runs the line function along rows instead of transposing
    uint32_t dist_timing = 0;        // ... k (measurements): the call brackets its k-th kernel with the timer's events (1 column, 2 line y, 3 line x; 4 .. 6 the second round; 7 stats or mask)
    uint32_t split_timing = 0;       // vk_split_components (grids: label_max_blocks, dist_max_blocks): k (measurements): the call brackets its k-th phase with the timer's events (vk_launch_split.hip)
    uint32_t measure_timing = 0;     // vk_measure_components (grids: label_max_blocks): k (measurements): the call brackets its k-th phase with the timer's events (vk_launch_measure.hip)
    uint32_t thick_max_blocks = 0;   // vk_local_thickness: cap of its own grids (0: none; the borrowed distance kernels keep dist_max_blocks) -- lets a small volume drive the grid-stride loops over tiles and voxels
    uint32_t thick_timing = 0;       // ... k (measurements): the call brackets its k-th phase with the timer's events (vk_launch_thick.hip)
    uint32_t geo_max_blocks = 0;     // vk_geodesic_distance: cap of its grids (0: none) -- lets a small volume drive the grid-stride loops over tiles and voxels
    uint32_t geo_timing = 0;         // ... k (measurements): the call brackets its k-th phase with the timer's events; 9: it leaves its round counts as the last message (vk_launch_geo.hip)
    uint32_t skel_max_blocks = 0;    // vk_skeletonize: cap of its grids (0: none) -- lets a small volume drive the grid-stride loops over tiles and voxels
    uint32_t skel_timing = 0;        // ... k (measurements): the call brackets its k-th phase with the timer's events; 9: it leaves its iteration counts as the last message (vk_launch_skel.hip)
    uint32_t diff_max_blocks = 0;    // vk_steady_diffusion: cap of its grids (0: none) -- lets a small volume drive the grid-stride loops over tiles, voxels and face voxels
    uint32_t diff_timing = 0;        // ... k (measurements): the call brackets its k-th phase with the timer's events; 9: it leaves its block counts as the last message (vk_launch_diff.hip)
    uint32_t diff_lds = 0;           // ... 1 (measurements, tests): the sweeps stage each tile and its halo in LDS instead of loading neighbours from global memory; the same bits
    uint32_t resample_max_blocks = 0;  // vk_volume_resample: cap of the grid (0: none) -- lets a small volume drive the loop over tiles
    uint32_t resample_area_passes = 0; // ... 1 (measurements, tests): AREA as three axis passes through f32 intermediates instead of the fused footprint loop
    uint32_t resample_area_unroll = 1; // ... 0 (measurements, tests): AREA by an integer ratio of 2 .. 4 runs the table-driven footprint loops, not the unrolled ones
    uint32_t resample_timing = 0;      // ... 1 (measurements): the call brackets its kernel with the timer's events (the pass has one phase)

    // present targets (next row N1/N2)
    uint32_t *rgba8 = nullptr, *bgra8 = nullptr;
    uint32_t present_w = 0, present_h = 0;

    // Frames in flight (vk_ctx_frames_in_flight; vk_context.hip).  A slot owns a frame's surface: backbuffer, step image,
    // present targets, the stream its work runs on and the event that marks its end.  The CURRENT slot's surface lives in the
    // fields above (backbuffer, steps, rgba8, bgra8, present_w/h, stream) -- every other translation unit keeps addressing
    // those -- and is parked in its FrameSlot while another slot is current (frame_slot_switch).  fif_k == 1: one slot, on
    // whatever stream the context runs on.
    struct FrameSlot {
        void *backbuffer = nullptr;
        uint32_t *steps = nullptr, *rgba8 = nullptr, *bgra8 = nullptr;
        void *geom = nullptr;
        void *slice_values = nullptr;
        uint32_t present_w = 0, present_h = 0;
        hipStream_t stream = nullptr;  // fif_k > 1: the slot's stream, created with the ring at the highest stream priority (vk_ctx_frames_in_flight)
        hipEvent_t done = nullptr;     // recorded by vk_frame_end
        uint64_t id = 0;               // the frame the slot holds (0: none)
        bool ended = false;            // ... and whether vk_frame_end has recorded `done` for it
    } fif[VK_MAX_FRAMES_IN_FLIGHT];
    uint32_t fif_k = 1, fif_cur = 0;
    uint32_t fif_concurrent = 0;  // frames of the ring that may EXECUTE at once (vk_frame_begin); 0: k - 1 for k >= 3 -- one frame always waits, recorded, in its queue
    uint64_t fif_seq = 0;       // frames begun since the ring was sized: frame number n takes slot n % fif_k
    uint64_t fif_last_id = 0;   // ids handed out so far (never reused by a context)
    bool fif_open = false;      // between vk_frame_begin and vk_frame_end

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing_open = false, timing_done = false;

    // multi-GPU: this context's RCCL communicator (vk_comm_init_rank / vk_group_create)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_size = 0;
    bool comm_owned = false;
    bool in_group = false;  // a member of a vk_group: its communicator belongs to the group's world
};

// ---- errors --------------------------------------------------------------------------------------------
extern thread_local std::string g_create_err;  // errors of calls that have no context yet (vk_last_error(NULL))

inline int fail(vk_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg; else g_create_err = msg;
    return code;
}

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            return fail(ctx, e_ == hipErrorOutOfMemory ? VK_ERR_OOM : VK_ERR_HIP,              \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                    \
        }                                                                                      \
    } while (0)

// ---- allocations ----------------------------------------------------------------------------------------
// Every device and pinned-host allocation the library makes on behalf of a context goes through these two (the counters of vk_ctx_create,
// made before there is a context, and vk_group_render's buffers, which belong to no context, do not).  On failure *p is NULL and HIP's
// sticky last error is cleared -- the caller reports the code it gets, and no later look at hipGetLastError() behind a launch finds it --
// and the call site keeps its own message and clean-up.  The allocation the debug hook picks (vk_alloc_hook.hpp) asks the runtime for
// kAllocRefused bytes in place of its own size: more than any device holds, so the code and the runtime's state are those of a real refusal.
constexpr size_t kAllocRefused = (size_t)1 << 60;
inline hipError_t ctx_alloc(vk_ctx *ctx, void **p, size_t bytes) {
    *p = nullptr;
    const hipError_t e = hipMalloc(p, ctx->alloc_fail.fires() ? kAllocRefused : bytes);
    if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); }
    return e;
}
inline hipError_t ctx_alloc_host(vk_ctx *ctx, void **p, size_t bytes) {
    *p = nullptr;
    const hipError_t e = hipHostMalloc(p, ctx->alloc_fail.fires() ? kAllocRefused : bytes);
    if (e != hipSuccess) { *p = nullptr; (void)hipGetLastError(); }
    return e;
}
// ... and what a failed one returns: "prefix: what: <HIP's text>", VK_ERR_OOM where the runtime says out of memory
inline int alloc_failed(vk_ctx *ctx, hipError_t e, const std::string &prefix, const char *what) {
    return fail(ctx, e == hipErrorOutOfMemory ? VK_ERR_OOM : VK_ERR_HIP, prefix + ": " + what + ": " + hipGetErrorString(e));
}

// A hipMalloc'd temporary of one call: freed when the call returns, whichever way; release() hands the pointer on (install_dense).
struct DeviceTemp {
    void *p = nullptr;
    DeviceTemp() = default;
    DeviceTemp(DeviceTemp &&o) noexcept : p(o.release()) {}
    DeviceTemp(const DeviceTemp &) = delete;
    DeviceTemp &operator=(const DeviceTemp &) = delete;
    ~DeviceTemp() { if (p) (void)hipFree(p); }
    void *release() { void *q = p; p = nullptr; return q; }
};

// the context's volume as the kernels' argument
inline vk::VolumeDesc volume_desc(const vk_ctx *ctx) {
    vk::VolumeDesc V = ctx->vdesc;
    V.data = ctx->vol; V.data2 = ctx->vol2; V.dist = ctx->dist; V.lut = ctx->lut;
    V.nx = ctx->nx; V.ny = ctx->ny; V.nz = ctx->nz;
    V.nbx = ctx->nbx; V.nby = ctx->nby; V.nbz = ctx->nbz;
    return V;
}

// Frames in flight: how many of the ring's frames execute at once (vk_frame_begin holds the others back), and whether the launch being recorded
// belongs to a frame of a CROWDED ring -- three executing (k = 4) -- where the machine is full and the leaner kernel variants win.
inline uint32_t frames_concurrent(const vk_ctx *ctx) { return ctx->fif_concurrent ? ctx->fif_concurrent : (ctx->fif_k >= 3u ? ctx->fif_k - 1u : ctx->fif_k); }
inline bool frames_crowded(const vk_ctx *ctx) { return ctx->fif_open && ctx->fif_k > 1u && frames_concurrent(ctx) >= 3u; }

// the kernel's scale of a scalar volume format (vk_tf.hpp)
inline vk::SampleScale format_scale(int format) { return format == VK_FMT_R8_UNORM ? vk::SCALE_R8 : (format == VK_FMT_R16_UNORM ? vk::SCALE_U16 : vk::SCALE_VALUE); }

inline size_t px_bytes(int fmt) { return fmt == VK_OUT_RGBA16F ? 8 : 16; }
// a pixel of a partition's compact tiles: the backbuffer's pixel, or its three colour channels (VK_WIRE_RGB)
inline size_t wire_px_bytes(int fmt, int wire) { return wire == VK_WIRE_RGB ? px_bytes(fmt) / 4 * 3 : px_bytes(fmt); }

// ---- shared between translation units --------------------------------------------------------------------
int rebuild_skip_maps(vk_ctx *ctx, const uint32_t *d_prefix, uint32_t n, float lo, float hi, int projection, const float *iso = nullptr);  // vk_volume.hip: the current volume's maps under a table (nullptr: built-in) and a projection, or under an isosurface (iso: its threshold in sample values; nullptr: none)
int frames_drain(vk_ctx *ctx);   // vk_context.hip: wait for the work of every frame slot (one stream when fif_k == 1)
void free_volume(vk_ctx *ctx);   // vk_volume.hip
int install_dense(vk_ctx *ctx, void *d_dense, uint32_t nx, uint32_t ny, uint32_t nz, int format, int layout);  // vk_volume.hip: a dense device array of the context's own becomes its volume (adopted or freed, also on failure), under the state in force
void comm_release(vk_ctx *ctx);  // vk_comm.hip

// vk_order.hip: screen-space geometry of a camera, the tile order and its device ring
void cull_rect_cam(const vk_ctx *ctx, const float *cam, int mode, int32_t r[4]);  // (rectangle and order below: of the context's clip box, if one is set)
void clip_key(const vk_ctx *ctx, uint32_t k[7]);  // the clip box as part of a cached order's key
void compute_tile_order_raw(const vk_ctx *ctx, const float *cam, int mode, int32_t ox, int32_t oy, uint32_t rw, uint32_t rh, uint32_t ts,
                            uint32_t *order, uint32_t *order_pos, uint32_t &order_active, int G);
int tile_order_update(vk_ctx *ctx, int mode, int32_t ox, int32_t oy, uint32_t rw, uint32_t rh, uint32_t ts, bool need_device);
int order_ensure_device(vk_ctx *ctx);
int order_wait(vk_ctx *ctx);

// vk_post.hip
int present_targets(vk_ctx *ctx, uint32_t width, uint32_t height, bool also_bgra);

// vk_render.hip
int check_render(vk_ctx *ctx, int mode, const float *cam, float dt_scale, uint32_t ts, uint32_t rank, uint32_t nranks);
int dispatch_march(vk_ctx *ctx, int mode, const vk::LaunchDesc &L_in, uint32_t flags, const float *reach_cam, const vk::GeomDesc *geom = nullptr);  // geom: the geometry pass of the isosurface (vk_render_geometry)
uint32_t launch_flags(const vk_ctx *ctx, uint32_t render_flags, bool batch);

// the kernel-instantiating TUs: each launches on ctx->stream and returns; the caller checks hipGetLastError
void launch_cells(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, uint32_t grid, bool count, bool skip, bool safe, int walk /* vk_march.hpp: WalkKind */);
void launch_cells_tf(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::TfDesc &T, const vk::ClipDesc *Cl /* nullptr: no box */, uint32_t grid, bool count, bool skip, bool safe);  // vk_launch_tf.hip
void launch_cells_lit(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::TfDesc &T, const vk::LightDesc &Lt, const vk::ClipDesc *Cl /* nullptr: no box */, uint32_t grid, bool count, bool skip,
                      bool safe);  // vk_launch_lit.hip
void launch_cells_mip(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::TfDesc &T, const vk::ClipDesc *Cl /* nullptr: no box */, uint32_t grid, bool count, bool skip, bool safe);  // vk_launch_mip.hip (T.rgba == nullptr: the grey ramp)
void launch_cells_iso(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::IsoDesc &I, const vk::ClipDesc *Cl /* nullptr: no box */, uint32_t grid, bool count, bool skip, bool safe);  // vk_launch_iso.hip
void launch_cells_iso_shadow(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::IsoDesc &I, const vk::ShadowDesc &Sh, const vk::ClipDesc *Cl /* nullptr: no box */, uint32_t grid, bool count,
                             bool skip, bool safe);  // vk_launch_iso_shadow.hip
void launch_u16_iso_shadow(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::IsoDesc &I, const vk::ShadowDesc &Sh, const vk::ClipDesc *Cl /* nullptr: no box */, uint32_t grid, bool count,
                           bool skip, bool safe);  // vk_launch_u16_iso_shadow.hip
void launch_cells_geom(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::IsoDesc &I, const vk::GeomDesc &G, const vk::ClipDesc *Cl /* nullptr: no box */, uint32_t grid, bool skip,
                       bool safe);  // vk_launch_geom.hip
void launch_u16_geom(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::IsoDesc &I, const vk::GeomDesc &G, const vk::ClipDesc *Cl /* nullptr: no box */, uint32_t grid, bool skip,
                     bool safe);  // vk_launch_u16_geom.hip
void launch_slice(vk_ctx *ctx, const vk::VolumeDesc &V, const vk::SliceDesc &S);  // vk_launch_slice.hip
// vk_launch_u16_*.hip: the same five families on an R16_UNORM volume (vk_march_u16.hpp); a family reads its own descriptors, Cl == nullptr: no box
#define VK_U16_LAUNCH(name) void name(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, const vk::TfDesc &T, const vk::LightDesc &Li, const vk::IsoDesc &I, const vk::ClipDesc *Cl, uint32_t grid, bool count, bool skip, bool safe)
VK_U16_LAUNCH(launch_u16_cells);
VK_U16_LAUNCH(launch_u16_tf);
VK_U16_LAUNCH(launch_u16_lit);
VK_U16_LAUNCH(launch_u16_mip);
VK_U16_LAUNCH(launch_u16_iso);
#undef VK_U16_LAUNCH
void launch_staged(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, uint32_t grid, bool count, const float *cam);
void launch_compute(vk_ctx *ctx, const vk::LaunchDesc &L, const vk::VolumeDesc &V, uint32_t grid, bool count, bool records, bool skip);
void launch_procedural(vk_ctx *ctx, const vk::LaunchDesc &L, uint32_t grid, bool count, float time, bool device_sine);
