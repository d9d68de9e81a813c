// bonsai.cpp -- headless counterpart of `cargo run --example bonsai` (examples/bonsai/main.rs):
// the same Demo (volume + raycast pipeline), the same camera, rendered N frames into the backbuffer.
//   bonsai [--frames N] [--size WxH] [--dt S] [--raw bonsai_256x256x256_uint8.raw] [--ppm out.ppm]
//          [--raw-u16 FILE] [--dims NX NY NZ]                 a raw volume of native-endian 16-bit integers, uploaded as R16_UNORM (CT / MR data);
//                                                            --dims: the voxel dims of --raw / --raw-u16 (default 256 256 256)
//          [--f32] [--dump-rgba file] [--dump-steps file]   parity surface (rgba32f) + per-pixel trip counts, raw
//          [--gpus N] [--batch B] [--peer-direct]            the frame's tiles over N GPUs of this node (vk_group_*); --peer-direct: the GPUs
//                                                            store into GPU 0's frames themselves instead of gather + un-tile
//          [--in-flight K] [--orbit] [--fuse-present] [--record]                        K frames in flight (vk_ctx_frames_in_flight); --orbit: the camera turns by 2 pi / 1024 every frame;
//                                                            --record: capture_frame of every frame, K - 1 frames behind (the recorder, src/lib.rs:196-199)
//          [--tf table.f32 [--tf-domain LO HI]]               runtime transfer function (vk_set_transfer_function): raw little-endian f32
//                                                            RGBA rows, 2..256 of them, over the sample values [LO, HI] (default 0 1)
//          [--light X Y Z | --headlight] [--light-params KA KD KS N]   gradient lighting of the table (vk_set_lighting; needs --tf): a light
//                                                            towards (X, Y, Z) or at the eye; ambient, diffuse, specular, shininess (default 0.3 0.7 0.2 32)
//          [--mip]                                            maximum-intensity projection (vk_set_projection(VK_PROJ_MAX)) over the table's window,
//                                                            without --tf a grey ramp over [0, 1]
//          [--iso V [--iso-colour R G B] [--iso-refine N]]    first-hit isosurface at sample value V (vk_set_isosurface): linear surface colour
//                                                            (default 1 1 1), N bisection steps at the hit (default 4); shaded by --light /
//                                                            --headlight (no --tf needed); refused together with --mip
//          [--shadows STRENGTH BIAS]                          light-direction shadows of the lit isosurface (vk_set_shadows; with --iso and --light): a shadowed
//                                                            point loses STRENGTH (0 .. 1) of its diffuse and specular terms; BIAS: first shadow sample, in steps
//          [--pick X Y]                                       what the ray through pixel (X, Y) of the last frame hits (vk_pick; needs --iso): the
//                                                            crossing, its distance along the ray, the gradient, the outward normal -g / |g|, the value
//          [--depth-ppm FILE]                                 the geometry pass of the last frame (vk_render_geometry; needs --iso) as a grey ramp of t between
//                                                            the frame's smallest (white) and largest (dark grey) finite t, misses black
//          [--clip X0 Y0 Z0 X1 Y1 Z1]                         clip box (cut-away) in unit-cube coordinates (vk_set_clip_box): the rays march the box
//                                                            only; needs --tf, --mip or --iso
//          [--slice AXIS POS | --slice-plane CX CY CZ NX NY NZ EXTENT]   the slice pass in place of the raycast (vk_render_slice): the plane AXIS = POS
//                                                            (AXIS x | y | z, POS in 0 .. 1) fitted into the frame, or the plane through (CX, CY, CZ) with
//                                                            normal (NX, NY, NZ) whose frame is EXTENT wide, in units of the volume's longest side; pixels
//                                                            are square in voxel space.  With either: --ppm, --tf, --raw / --raw-u16, --dims, --clip, and
//          [--slab SAMPLES THICKNESS max|min|mean]            a thick slab: SAMPLES (1 .. 256) planes over THICKNESS along the normal, reduced
//          [--histogram BINS [LO HI]]                         in place of the raycast (vk_volume_histogram): the statistics of the volume and one `bin count` line per
//                                                            non-empty bin of BINS (1 .. 4096) bins over the sample values [LO, HI] (default 0 1)
//          [--auto-window P_LO P_HI]                          before the first frame, the table's domain -- of --tf, or of the grey ramp of --mip / --slice -- becomes the
//                                                            window that holds the percentiles P_LO .. P_HI (0 <= P_LO < P_HI <= 1) of a 4096-bin histogram over
//                                                            [0, 1] (vk_histogram_window); needs --tf, --mip, --slice or --slice-plane
//          [--mesh OUT.stl|OUT.obj [--mesh-iso V] [--mesh-scale SX SY SZ]]   in place of the raycast (vk_extract_isosurface): the isosurface at sample value V
//                                                            (default: --iso's) as binary STL or welded OBJ, the unit cube scaled by SX SY SZ (default 1 1 1);
//                                                            honours --clip (the voxels whose centres lie in the box), --raw / --raw-u16 and --dims
//          [--crop X0 Y0 Z0 X1 Y1 Z1 | clip] [--resample NX NY NZ [nearest|linear|area]] [--downsample F] [--isotropic SX SY SZ] [--to-u8 LO HI] [--to-u16 LO HI]
//                                                            the resample pass (vk_volume_resample), as installing calls right after the volume is loaded, before
//                                                            --median / --smooth, in the order given (up to 16): --crop keeps the voxels of a box (clip: of the --clip
//                                                            box, which is then turned off), --resample resizes to NX NY NZ (0: that axis stays; default linear),
//                                                            --downsample F takes the mean of F^3 voxels (area, 1 .. 16), --isotropic resizes a scan of voxel
//                                                            spacing SX SY SZ to cubic voxels (linear), --to-u8 / --to-u16 map the sample values LO .. HI onto the
//                                                            whole range of the new format (nearest, same size; either may stand beside a resize).  Every later
//                                                            flag sees the new volume; the new dimensions and format are printed; --save-raw writes the new array
//          [--median] [--smooth SX SY SZ] [--save-raw PATH]    the volume filter pass (vk_volume_filter), applied once the volume is loaded and before anything else,
//                                                            so --iso, --mesh, --histogram and --auto-window see the filtered data: first the 3x3x3 median,
//                                                            then a Gaussian of SX SY SZ voxels (0: the axis is skipped); --save-raw writes the filtered dense
//                                                            volume, x fastest, in the volume's format (needs --median or --smooth; one GPU)
//          [--components LO HI [CONN]]                        connected components of the voxels whose stored texel lies in the sample values [LO, HI] (HI may be inf;
//                                                            vk_label_components), connectivity CONN = 6 (default), 18 or 26: prints the totals and the ten largest;
//                                                            runs after --median / --smooth and before --histogram, --auto-window, --mesh, --save-raw and the frames
//          [--keep-largest K] [--drop-islands N] [--keep-voxel X Y Z] [--remove-voxel X Y Z] [--keep-pick PX PY] [--label-fill V]
//                                                            keep or drop components of that range (each flag up to 16 times; they need --components, or --iso V
//                                                            for the range [V, inf) at connectivity 6), in this order: the components under the --remove-voxel
//                                                            voxels become the fill; only those under the --keep-voxel voxels and --keep-pick pixels stay
//                                                            (--keep-pick: what the ray through pixel (PX, PY) hits; needs --iso); components below N voxels go;
//                                                            the K largest stay.  A voxel that goes becomes the sample value V of --label-fill (default 0).  The
//                                                            cleaned volume replaces the loaded one; --save-raw writes it
//          [--morph close|open|dilate|erode RADIUS] [--morph-spacing SX SY SZ] [--morph-fill IN OUT]
//                                                            morphology of that range by a Euclidean ball (vk_distance_transform; up to 16 times, in the order
//                                                            given): RADIUS in the units of the integer voxel pitch SX SY SZ (default 1 1 1); a voxel that joins
//                                                            the range becomes the sample value IN (default: HI, or max(LO, 1) under an open range), one that
//                                                            leaves it OUT (default 0).  Runs after --median / --smooth and before --components and the keep
//                                                            flags, so close-then-keep-largest and open-then-label both work; --save-raw writes the result
//          [--split RADIUS [CONN]]                          split touching objects of that range (vk_split_components): markers that survive an erosion by RADIUS
//                                                            (in the units of --morph-spacing) grow back over the range, and a voxel beside a region of smaller id
//                                                            becomes the sample value of --label-fill (default 0).  CONN: 6 (default), 18 or 26.  Runs after --morph
//                                                            and before --components and the keep flags, so --split 6 --keep-pick PX PY isolates the one grain under
//                                                            a pixel; prints the totals and the ten largest regions; --save-raw writes the cut volume
//          [--measure [FILE.csv]]                           measure the regions of that range (vk_measure_components): the components of [LO, HI] (--components, or
//                                                            --iso V for [V, inf) at connectivity 6) on the volume that --morph, --split and the keep flags left -- after
//                                                            --split, the split regions.  Prints the totals and the ten largest regions: id, voxels, centroid,
//                                                            equivalent diameter, principal lengths, mean +- std, surface, in the units of --morph-spacing; FILE.csv
//                                                            takes one line per region
//          [--thickness MAX_RADIUS [GAIN]]                  local thickness of that range (vk_local_thickness): every voxel of the range takes the radius of the largest
//                                                            ball that fits inside the range and holds it, capped at MAX_RADIUS (in the units of --morph-spacing), stored
//                                                            as radius * GAIN (default: the thickest place stores full scale); every other voxel becomes the sample value
//                                                            of --label-fill (default 0).  Runs after --measure, as the last step that replaces the volume, so
//                                                            --thickness 16 --histogram 64 prints the thickness distribution and --thickness 16 --tf table.f32 renders
//                                                            the range coloured by thickness; prints the totals; --save-raw writes the thickness map
//          [--geodesic FACE [TARGET_FACE]] [--geodesic-voxel X Y Z]...   geodesic distance through that range (vk_geodesic_distance): every voxel of the range takes the length of the
//                                                            shortest path inside the range from the voxels of the range on FACE (x- x+ y- y+ z- z+) and from the
//                                                            --geodesic-voxel seeds (at most 16; either flag may stand alone), over steps to the 26 neighbours (or
//                                                            --components' CONN) in the units of --morph-spacing; the farthest reached voxel stores full scale, an
//                                                            unreached voxel and every voxel outside the range the sample value of --label-fill (default 0).  Runs
//                                                            after --thickness, as the last step that replaces the volume; prints foreground, sources, reached,
//                                                            unreached, largest and mean distance, and with TARGET_FACE "percolates yes|no", the target distance and
//                                                            the tortuosity along that face's axis; --save-raw writes the distance map
//          [--skeleton [curve|kernel] [MAX_ITER]]           skeleton of that range (vk_skeletonize): the range thinned to a one-voxel-wide set with the same pieces, tunnels
//                                                            and cavities; curve (the default) keeps line ends and gives centre lines, kernel thins to the ultimate
//                                                            homotopic kernel; MAX_ITER stops after that many iterations (default 0: until nothing more can go).  The
//                                                            skeleton keeps its stored values -- after --thickness the radius along each centre line --, every other
//                                                            voxel takes the sample value of --label-fill (default 0).  Runs after --geodesic, as the last step that
//                                                            replaces the volume; prints foreground, skeleton voxels, ends, junctions, isolated voxels and the length in
//                                                            the units of --morph-spacing; --save-raw writes the skeleton
//          [--diffusion AXIS [MAX_SWEEPS]] [--diffusion-install]   steady-state diffusion through that range (vk_steady_diffusion): the Laplace equation on the range with no-flux
//                                                            walls, concentration 1 on the first plane along AXIS (x y z) and 0 on the last, in the pitch of
//                                                            --morph-spacing, at most MAX_SWEEPS sweeps (default 20000).  Runs after --skeleton, as the last analysing
//                                                            step; prints foreground, porosity, sweeps, "converged yes|no", the flux in and out, D_eff/D0 and the
//                                                            tortuosity factor.  --diffusion-install: the concentration field replaces the volume (every voxel outside
//                                                            the range takes --label-fill), so that --tf renders it and --save-raw writes it
//          [--camera-blobs orbits.txt out.bin]              no GPU: one 144-byte CameraUniform per "zoom pitch yaw tx ty tz aspect" line
#include <cstdio>
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "vokselis.hpp"

using namespace vokselis;

static std::string g_raw;
static int g_raw_fmt = VK_FMT_R8_UNORM;  // --raw-u16: VK_FMT_R16_UNORM
static uint32_t g_dims[3] = {256, 256, 256};  // --dims
static float g_dt = 1.0f;
static bool g_orbit = false;
static std::vector<float> g_tf;  // --tf: n x 4 floats (empty: the built-in transfer)
static float g_tf_lo = 0.0f, g_tf_hi = 1.0f;
static bool g_lit = false;  // --light / --headlight: gradient lighting (the library checks the parameters)
static bool g_mip = false;  // --mip: maximum-intensity projection
static bool g_iso_on = false;  // --iso: first-hit isosurface (the library checks the parameters)
static vk_isosurface g_iso = {0.0f, {1.0f, 1.0f, 1.0f}, 4u};
static bool g_shadows_on = false;  // --shadows: light-direction shadows (the library checks the parameters)
static vk_shadows g_shadows = {0.7f, 2.0f};
static bool g_clip_on = false;  // --clip: clip box (the library checks the bounds)
static vk_clip_box g_clip = {{0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}};
static vk_lighting g_light = {{0.0f, 0.0f, 0.0f}, 0, 0.3f, 0.7f, 0.2f, 32.0f};
static bool g_auto_window = false;  // --auto-window: the table's domain from the volume's percentiles
static double g_auto_lo = 0.0, g_auto_hi = 1.0;

static bool g_median = false;      // --median: the 3x3x3 median of the loaded volume
static bool g_smooth = false;      // --smooth: then a Gaussian of g_sigma voxels per axis
static double g_sigma[3] = {0.0, 0.0, 0.0};
static std::string g_save_raw;     // --save-raw: the filtered dense volume
// --crop, --resample, --downsample, --isotropic, --to-u8, --to-u16 (vk_volume_resample), in the order given
struct ResampleOp {
    enum Kind { CROP, CROP_CLIP, RESIZE, DOWNSAMPLE, ISOTROPIC, CONVERT } kind;
    const char *name;
    vk_voxel_box box;      // CROP
    uint32_t dims[3];      // RESIZE; DOWNSAMPLE: the factor in dims[0]
    int mode;              // RESIZE
    double spacing[3];     // ISOTROPIC
    int format;            // CONVERT
    float window[2];       // CONVERT
};
static std::vector<ResampleOp> g_resample;

// --components and the keep flags (vk_label_components)
static bool g_components = false;  // --components LO HI [CONN]
static float g_label_lo = 0.0f, g_label_hi = INFINITY, g_label_fill = 0.0f;
static uint32_t g_label_conn = 6;
static bool g_label_fill_on = false;
static std::vector<uint64_t> g_keep_largest, g_drop_islands;                      // --keep-largest K, --drop-islands N, in the order given
static std::vector<std::array<uint32_t, 3>> g_keep_voxels, g_remove_voxels;      // --keep-voxel, --remove-voxel
static std::vector<std::array<uint32_t, 2>> g_keep_picks;                        // --keep-pick PX PY
static uint32_t g_w = 1280, g_h = 720;                                           // --size: --keep-pick's pixels are this frame's
// --morph (vk_distance_transform), on the same range
struct MorphOp { int op; const char *name; float radius; };
static std::vector<MorphOp> g_morph;                                             // --morph OP RADIUS, in the order given
static uint32_t g_morph_spacing[3] = {1u, 1u, 1u};                               // --morph-spacing SX SY SZ
static float g_morph_fill[2] = {0.0f, 0.0f};                                     // --morph-fill IN OUT
static bool g_morph_spacing_on = false, g_morph_fill_on = false;
static bool g_split_on = false;                                                  // --split RADIUS [CONN] (vk_split_components), on the same range
static float g_split_radius = 0.0f;
static uint32_t g_split_conn = 6;
static bool g_measure_on = false;                                                // --measure [FILE.csv] (vk_measure_components), on the same range
static std::string g_measure_csv;
static bool g_thick_on = false;                                                  // --thickness MAX_RADIUS [GAIN] (vk_local_thickness), on the same range
static float g_thick_radius = 16.0f, g_thick_gain = 0.0f;                        // (gain 0: automatic)
static bool g_geo_on = false;                                                    // --geodesic FACE [TARGET_FACE], --geodesic-voxel X Y Z (vk_geodesic_distance), on the same range
static bool g_geo_face_on = false, g_label_conn_on = false;                      // (--components gave a CONN: the geodesic steps follow it, else 26)
static uint32_t g_geo_sources = 0, g_geo_targets = 0;
static int g_geo_axis = 0;                                                       // the target face's axis
static std::vector<std::array<uint32_t, 3>> g_geo_seeds;
static bool g_skel_on = false;                                                   // --skeleton [curve|kernel] [MAX_ITER] (vk_skeletonize), on the same range
static uint32_t g_skel_mode = VK_SKEL_CURVE, g_skel_max_iter = 0;
static bool g_diff_on = false, g_diff_install = false, g_diff_save = false;      // --diffusion AXIS [MAX_SWEEPS], --diffusion-install (vk_steady_diffusion), on the same range; save: it fills --save-raw's file
static uint32_t g_diff_axis = 0, g_diff_max_sweeps = 20000;
static bool label_ops() { return !g_keep_largest.empty() || !g_drop_islands.empty() || !g_keep_voxels.empty() || !g_remove_voxels.empty() || !g_keep_picks.empty(); }

// the context of a run that replaces the render: 8 x 8, or the frame's size under the render's camera when --keep-pick casts rays through it
static HdrBackBuffer pass_backbuffer() { HdrBackBuffer bb; bb.width = g_keep_picks.empty() ? 8u : g_w; bb.height = g_keep_picks.empty() ? 8u : g_h; return bb; }
static Camera pass_camera() { return Camera(1.f, 0.5f, 1.f, {0.5f, 0.5f, 0.5f}, (float)g_w / (float)g_h); }

static void write_dense(const std::vector<unsigned char> &dense, const char *what) {
    std::ofstream f(g_save_raw, std::ios::binary);
    if (!f || !f.write(reinterpret_cast<const char *>(dense.data()), (std::streamsize)dense.size())) throw std::runtime_error("cannot write " + g_save_raw);
    std::printf("%s volume: %zu bytes -> %s\n", what, dense.size(), g_save_raw.c_str());
}

// --morph, in the order given, after the filters and before --components and the keep flags; the last of them fills --save-raw's file unless a keep flag follows
static void apply_morph(Context &ctx) {
    if (g_morph.empty()) return;
    uint32_t dims[3] = {0, 0, 0};
    int fmt = 0;
    check(ctx.handle(), vk_volume_info(ctx.handle(), dims, &fmt, nullptr, nullptr));
    std::vector<unsigned char> dense;
    if (!g_save_raw.empty() && !label_ops() && !g_split_on && !g_thick_on && !g_geo_on && !g_skel_on && !g_diff_save) dense.resize((size_t)dims[0] * dims[1] * dims[2] * (fmt == VK_FMT_R8_UNORM ? 1u : 2u));
    const float fill_in = g_morph_fill_on ? g_morph_fill[0] : (std::isfinite(g_label_hi) ? g_label_hi : (std::isfinite(g_label_lo) ? std::max(g_label_lo, 1.0f) : 1.0f));
    for (size_t k = 0; k < g_morph.size(); k++) {
        const MorphOp &op = g_morph[k];
        const vk_distance_result r = ctx.morph_volume(g_label_lo, g_label_hi, op.op, op.radius, g_morph_spacing, fill_in, g_morph_fill[1], nullptr, false, true,
                                                      k + 1 == g_morph.size() && !dense.empty() ? dense.data() : nullptr);
        std::printf("morph %s %g: %llu voxels in the range, %llu afterwards (%llu added, %llu removed)\n", op.name, op.radius, (unsigned long long)r.n_foreground,
                    (unsigned long long)r.n_result, (unsigned long long)r.n_added, (unsigned long long)r.n_removed);
    }
    if (!dense.empty()) write_dense(dense, "morphed");
}

// --split, after --morph and before --components and the keep flags; it fills --save-raw's file unless a keep flag follows
static void apply_split(Context &ctx) {
    if (!g_split_on) return;
    uint32_t dims[3] = {0, 0, 0};
    int fmt = 0;
    check(ctx.handle(), vk_volume_info(ctx.handle(), dims, &fmt, nullptr, nullptr));
    std::vector<unsigned char> dense;
    if (!g_save_raw.empty() && !label_ops() && !g_thick_on && !g_geo_on && !g_skel_on && !g_diff_save) dense.resize((size_t)dims[0] * dims[1] * dims[2] * (fmt == VK_FMT_R8_UNORM ? 1u : 2u));
    const Regions r = ctx.split_components(g_label_lo, g_label_hi, g_split_radius, g_morph_spacing, g_split_conn, nullptr, false, false, g_label_fill, true, dense.empty() ? nullptr : dense.data());
    std::printf("split: [%g, %g] radius %g connectivity %u: %llu regions (%llu markers of %llu voxels, %llu unreached regions of %llu voxels), %llu foreground voxels, %llu cut, %u rounds\n",
                g_label_lo, g_label_hi, g_split_radius, g_split_conn, (unsigned long long)r.totals.n_regions, (unsigned long long)r.totals.n_markers, (unsigned long long)r.totals.n_marker_voxels,
                (unsigned long long)r.totals.n_residue_regions, (unsigned long long)r.totals.n_residue_voxels, (unsigned long long)r.totals.n_foreground, (unsigned long long)r.totals.n_cut, r.totals.rounds);
    for (uint64_t id : r.largest(10)) {
        const vk_component &k = r.table[id - 1];
        std::printf("region %llu: %llu voxels, anchor %llu, box %u %u %u .. %u %u %u\n", (unsigned long long)id, (unsigned long long)k.n_voxels, (unsigned long long)k.first, k.box.x0, k.box.y0, k.box.z0,
                    k.box.x1, k.box.y1, k.box.z1);
    }
    if (!dense.empty()) write_dense(dense, "split");
}

// --morph, then --split, then --components, then the keep flags in their fixed order, after the filters and before anything else reads the volume; the last of them fills --save-raw's file
static void apply_labels(Context &ctx) {
    apply_morph(ctx);
    apply_split(ctx);
    if (!g_components && !label_ops()) return;
    uint32_t dims[3] = {0, 0, 0};
    int fmt = 0;
    check(ctx.handle(), vk_volume_info(ctx.handle(), dims, &fmt, nullptr, nullptr));
    if (g_components) {
        const Components c = ctx.label_components(g_label_lo, g_label_hi, g_label_conn);
        std::printf("components: [%g, %g] connectivity %u: %llu components, %llu foreground voxels of %llu\n", g_label_lo, g_label_hi, g_label_conn,
                    (unsigned long long)c.totals.n_components, (unsigned long long)c.totals.n_foreground, (unsigned long long)dims[0] * dims[1] * dims[2]);
        for (uint64_t id : c.largest(10)) {
            const vk_component &k = c.table[id - 1];
            std::printf("component %llu: %llu voxels, first %llu, box %u %u %u .. %u %u %u\n", (unsigned long long)id, (unsigned long long)k.n_voxels, (unsigned long long)k.first, k.box.x0,
                        k.box.y0, k.box.z0, k.box.x1, k.box.y1, k.box.z1);
        }
    }
    if (!label_ops()) return;
    std::vector<std::array<uint32_t, 3>> keep = g_keep_voxels;
    if (!g_keep_picks.empty()) {  // the rays of the render's camera through the frame's pixels, under --iso
        const CameraUniform cu = ctx.camera.get_proj_view_matrix();
        check(ctx.handle(), vk_set_camera(ctx.handle(), &cu));
        ctx.set_isosurface(&g_iso);
        for (const auto &p : g_keep_picks) {
            const vk_hit hit = ctx.pick(p[0], p[1], g_dt);
            if (!hit.hit) { std::printf("keep-pick (%u, %u): miss\n", p[0], p[1]); continue; }
            keep.push_back(voxel_of(hit.pos, dims[0], dims[1], dims[2]));
            std::printf("keep-pick (%u, %u): voxel %u %u %u\n", p[0], p[1], keep.back()[0], keep.back()[1], keep.back()[2]);
        }
        if (keep.size() > (size_t)VK_LABEL_MAX_SEEDS) throw std::runtime_error("--keep-voxel and --keep-pick: at most 16 seeds together");
    }
    struct Op { const char *name; int keep; uint64_t count; const std::vector<std::array<uint32_t, 3>> *seeds; bool invert; };
    static const std::vector<std::array<uint32_t, 3>> none;
    std::vector<Op> ops;
    if (!g_remove_voxels.empty()) ops.push_back({"remove-voxel", VK_LABEL_KEEP_SEEDS, 0, &g_remove_voxels, true});
    if (!g_keep_voxels.empty() || !g_keep_picks.empty()) {
        if (keep.empty()) throw std::runtime_error("--keep-pick: every ray missed, nothing would be kept");
        ops.push_back({"keep-voxel", VK_LABEL_KEEP_SEEDS, 0, &keep, false});
    }
    for (uint64_t n : g_drop_islands) ops.push_back({"drop-islands", VK_LABEL_KEEP_MIN_SIZE, n, &none, false});
    for (uint64_t k : g_keep_largest) ops.push_back({"keep-largest", VK_LABEL_KEEP_LARGEST, k, &none, false});
    std::vector<unsigned char> dense;
    if (!g_save_raw.empty() && !g_thick_on && !g_geo_on && !g_skel_on && !g_diff_save) dense.resize((size_t)dims[0] * dims[1] * dims[2] * (fmt == VK_FMT_R8_UNORM ? 1u : 2u));
    for (size_t k = 0; k < ops.size(); k++) {
        const Op &op = ops[k];
        const vk_label_result r = ctx.keep_components(g_label_lo, g_label_hi, op.keep, op.count, *op.seeds, op.invert, g_label_fill, g_label_conn, nullptr, false, true,
                                                      k + 1 == ops.size() && !dense.empty() ? dense.data() : nullptr);
        std::printf("%s: %llu of %llu components selected, %llu of %llu foreground voxels\n", op.name, (unsigned long long)r.n_kept_components, (unsigned long long)r.n_components,
                    (unsigned long long)r.n_kept_voxels, (unsigned long long)r.n_foreground);
    }
    if (!dense.empty()) write_dense(dense, "cleaned");
}

// --measure, after --morph, --split, --components and the keep flags, on the volume they left
static void apply_measure(Context &ctx) {
    if (!g_measure_on) return;
    const Measurements m = ctx.measure_components(g_label_lo, g_label_hi, g_label_conn);
    const double sp[3] = {(double)g_morph_spacing[0], (double)g_morph_spacing[1], (double)g_morph_spacing[2]};
    std::printf("measure: [%g, %g] connectivity %u: %llu regions, %llu foreground voxels of %llu, spacing %g %g %g\n", g_label_lo, g_label_hi, g_label_conn, (unsigned long long)m.totals.n_regions,
                (unsigned long long)m.totals.n_foreground, (unsigned long long)m.dims[0] * m.dims[1] * m.dims[2], sp[0], sp[1], sp[2]);
    for (uint64_t id : m.largest(10)) {
        const size_t k = (size_t)id - 1;
        const std::array<double, 3> c = m.centroid(k), l = m.principal_lengths(k, sp);
        std::printf("region %llu: %llu voxels, centroid %.3f %.3f %.3f, diameter %.3f, lengths %.3f %.3f %.3f, mean %.6g +- %.6g, surface %.6g\n", (unsigned long long)id,
                    (unsigned long long)m.table[k].n_voxels, c[0], c[1], c[2], m.equivalent_diameter(k, sp), l[0], l[1], l[2], m.mean(k), m.stddev(k), m.surface_area(k, sp));
    }
    if (!g_measure_csv.empty()) {
        m.to_csv(g_measure_csv, sp);
        std::printf("measure: %zu regions -> %s\n", m.table.size(), g_measure_csv.c_str());
    }
}

// --thickness, after --measure: the last step that replaces the volume; it takes over --save-raw's file
static void apply_thickness(Context &ctx) {
    if (!g_thick_on) return;
    uint32_t dims[3] = {0, 0, 0};
    int fmt = 0;
    check(ctx.handle(), vk_volume_info(ctx.handle(), dims, &fmt, nullptr, nullptr));
    std::vector<unsigned char> dense;
    if (!g_save_raw.empty() && !g_geo_on && !g_skel_on && !g_diff_save) dense.resize((size_t)dims[0] * dims[1] * dims[2] * (fmt == VK_FMT_R8_UNORM ? 1u : 2u));
    const vk_thickness_result r = ctx.local_thickness(g_label_lo, g_label_hi, g_thick_radius, g_morph_spacing, nullptr, false, g_thick_gain, g_label_fill, true, dense.empty() ? nullptr : dense.data());
    std::printf("thickness: [%g, %g] cap %g spacing %u %u %u: %llu foreground voxels, largest thickness %.6g, %llu saturated voxels, gain %.9g\n", g_label_lo, g_label_hi, g_thick_radius,
                g_morph_spacing[0], g_morph_spacing[1], g_morph_spacing[2], (unsigned long long)r.n_foreground, Context::thickness_of(r.max_t2), (unsigned long long)r.n_saturated, r.gain);
    if (!dense.empty()) write_dense(dense, "thickness");
}

// --geodesic / --geodesic-voxel, after --thickness: the last step that replaces the volume; it takes over --save-raw's file
static void apply_geodesic(Context &ctx) {
    if (!g_geo_on) return;
    uint32_t dims[3] = {0, 0, 0};
    int fmt = 0;
    check(ctx.handle(), vk_volume_info(ctx.handle(), dims, &fmt, nullptr, nullptr));
    std::vector<unsigned char> dense;
    if (!g_save_raw.empty() && !g_skel_on && !g_diff_save) dense.resize((size_t)dims[0] * dims[1] * dims[2] * (fmt == VK_FMT_R8_UNORM ? 1u : 2u));
    const uint32_t conn = g_label_conn_on ? g_label_conn : 26u;
    const vk_geodesic_result r = ctx.geodesic_distance(g_label_lo, g_label_hi, g_geo_sources, g_geo_targets, g_geo_seeds, conn, g_morph_spacing, nullptr, false, 0.0f, g_label_fill, g_label_fill, true,
                                                       dense.empty() ? nullptr : dense.data());
    std::printf("geodesic: [%g, %g] connectivity %u spacing %u %u %u: %llu foreground voxels, %llu sources, %llu reached, %llu unreached, largest distance %.6g, mean distance %.6g\n", g_label_lo,
                g_label_hi, conn, g_morph_spacing[0], g_morph_spacing[1], g_morph_spacing[2], (unsigned long long)r.n_foreground, (unsigned long long)r.n_sources, (unsigned long long)r.n_reached,
                (unsigned long long)(r.n_foreground - r.n_reached), Context::geodesic_units(r.max_g), r.n_reached ? (double)r.sum_g / ((double)VK_GEO_UNIT * (double)r.n_reached) : 0.0);
    if (g_geo_targets) {
        const bool through = r.target_min != VK_GEO_INF;
        std::printf("geodesic: percolates %s", through ? "yes" : "no");
        if (through) {
            std::printf(", target distance %.6g", Context::geodesic_units(r.target_min));
            if (dims[g_geo_axis] > 1u) std::printf(", tortuosity %.6g along %c", Context::geodesic_units(r.target_min) / ((double)g_morph_spacing[g_geo_axis] * (double)(dims[g_geo_axis] - 1u)), "xyz"[g_geo_axis]);
        }
        std::printf("\n");
    }
    if (!dense.empty()) write_dense(dense, "geodesic");
}

// --skeleton, after --geodesic: the last step that replaces the volume; it takes over --save-raw's file
static void apply_skeleton(Context &ctx) {
    if (!g_skel_on) return;
    uint32_t dims[3] = {0, 0, 0};
    int fmt = 0;
    check(ctx.handle(), vk_volume_info(ctx.handle(), dims, &fmt, nullptr, nullptr));
    std::vector<unsigned char> dense;
    if (!g_save_raw.empty() && !g_diff_save) dense.resize((size_t)dims[0] * dims[1] * dims[2] * (fmt == VK_FMT_R8_UNORM ? 1u : 2u));
    const vk_skeleton_result r = ctx.skeletonize(g_label_lo, g_label_hi, g_skel_mode, g_skel_max_iter, nullptr, false, nullptr, g_label_fill, true, dense.empty() ? nullptr : dense.data());
    std::printf("skeleton: [%g, %g] %s spacing %u %u %u: %llu foreground voxels, %llu skeleton voxels, %llu ends, %llu junctions, %llu isolated voxels, length %.6g, %u iterations%s\n", g_label_lo,
                g_label_hi, g_skel_mode == VK_SKEL_KERNEL ? "kernel" : "curve", g_morph_spacing[0], g_morph_spacing[1], g_morph_spacing[2], (unsigned long long)r.n_foreground,
                (unsigned long long)r.n_skeleton, (unsigned long long)r.n_end, (unsigned long long)r.n_junction, (unsigned long long)r.n_isolated, Context::skeleton_length(r, g_morph_spacing),
                r.iterations, r.converged ? "" : " (stopped by MAX_ITER)");
    if (!dense.empty()) write_dense(dense, "skeleton");
}

// --diffusion, after --skeleton: the last analysing step; with --diffusion-install it replaces the volume and takes over --save-raw's file
static void apply_diffusion(Context &ctx) {
    if (!g_diff_on) return;
    uint32_t dims[3] = {0, 0, 0};
    int fmt = 0;
    check(ctx.handle(), vk_volume_info(ctx.handle(), dims, &fmt, nullptr, nullptr));
    std::vector<unsigned char> dense;
    if (g_diff_save) dense.resize((size_t)dims[0] * dims[1] * dims[2] * (fmt == VK_FMT_R8_UNORM ? 1u : 2u));
    const vk_diffusion_result r = ctx.steady_diffusion(g_label_lo, g_label_hi, g_diff_axis, g_morph_spacing, 0.0f, 32u, 1e-5f, 1e-3f, g_diff_max_sweeps < 32u ? 32u : g_diff_max_sweeps, nullptr, false, 0.0f,
                                                       g_label_fill, g_diff_install, dense.empty() ? nullptr : dense.data());
    const Context::DiffusionValues v = Context::diffusion_values(r, g_diff_axis, dims);
    std::printf("diffusion: [%g, %g] along %c spacing %u %u %u: %llu foreground voxels, porosity %.6g, %u sweeps, converged %s, flux in %.6g out %.6g, D_eff/D0 %.6g, tortuosity factor %.6g\n", g_label_lo,
                g_label_hi, "xyz"[g_diff_axis], g_morph_spacing[0], g_morph_spacing[1], g_morph_spacing[2], (unsigned long long)r.n_foreground, v.porosity, r.sweeps, r.converged ? "yes" : "no", v.flux_in,
                v.flux_out, v.effective_diffusivity, v.tortuosity_factor);
    if (!dense.empty()) write_dense(dense, "diffusion");
}

// --crop, --resample, --downsample, --isotropic, --to-u8, --to-u16 in the order given, right after the volume is loaded; the last of them fills --save-raw's
// file unless a filter, a --morph or a keep flag follows
static void apply_resample(Context &ctx) {
    if (g_resample.empty()) return;
    static const char *const fmt_name[] = {"R8_UNORM", "R16_FLOAT", "RGBA16F_PAIR", "R16_UNORM"};
    const bool save = !g_save_raw.empty() && !g_median && !g_smooth && !label_ops() && g_morph.empty() && !g_split_on && !g_thick_on && !g_geo_on && !g_skel_on && !g_diff_save;
    std::vector<unsigned char> dense;
    for (size_t k = 0; k < g_resample.size(); k++) {
        const ResampleOp &op = g_resample[k];
        std::vector<unsigned char> *out = save && k + 1 == g_resample.size() ? &dense : nullptr;
        vk_resample_result r{};
        switch (op.kind) {
            case ResampleOp::CROP: r = ctx.crop_volume(&op.box, true, out); break;
            case ResampleOp::CROP_CLIP:
                if (!g_clip_on) throw std::runtime_error("--crop clip needs --clip");
                r = ctx.crop_volume(nullptr, true, out);
                g_clip_on = false;  // the crop is what the box showed
                break;
            case ResampleOp::RESIZE: r = ctx.resample_volume(op.dims, op.mode, nullptr, false, VK_RESAMPLE_KEEP_FORMAT, nullptr, VK_LAYOUT_AUTO, true, out); break;
            case ResampleOp::DOWNSAMPLE: r = ctx.downsample_volume(op.dims[0], true, out); break;
            case ResampleOp::ISOTROPIC: r = ctx.isotropic_volume(op.spacing, VK_RESAMPLE_LINEAR, true, out); break;
            case ResampleOp::CONVERT: r = ctx.resample_volume(nullptr, VK_RESAMPLE_NEAREST, nullptr, false, op.format, op.window, VK_LAYOUT_AUTO, true, out); break;
        }
        std::printf("%s: volume %u x %u x %u %s\n", op.name, r.dims[0], r.dims[1], r.dims[2], fmt_name[r.format & 3]);
    }
    if (save) write_dense(dense, "resampled");
}

// --median, then --smooth, once the volume is there and before anything reads it; the last of them also fills --save-raw's file (unless a keep flag follows)
static void apply_filters(Context &ctx) {
    apply_resample(ctx);
    if (!g_median && !g_smooth) { apply_labels(ctx); apply_measure(ctx); apply_thickness(ctx); apply_geodesic(ctx); apply_skeleton(ctx); apply_diffusion(ctx); return; }
    std::vector<unsigned char> dense;
    if (!g_save_raw.empty() && !label_ops() && g_morph.empty() && !g_split_on && !g_thick_on && !g_geo_on && !g_skel_on && !g_diff_save) {
        uint32_t dims[3] = {0, 0, 0};
        int fmt = 0;
        check(ctx.handle(), vk_volume_info(ctx.handle(), dims, &fmt, nullptr, nullptr));
        dense.resize((size_t)dims[0] * dims[1] * dims[2] * (fmt == VK_FMT_R8_UNORM ? 1u : 2u));
    }
    if (g_median) ctx.median_volume(true, g_smooth || dense.empty() ? nullptr : dense.data());
    if (g_smooth) ctx.smooth_volume(g_sigma[0], g_sigma[1], g_sigma[2], true, dense.empty() ? nullptr : dense.data());
    std::printf("filter:%s%s\n", g_median ? " median 3x3x3" : "", g_smooth ? (" gaussian sigma " + std::to_string(g_sigma[0]) + " " + std::to_string(g_sigma[1]) + " " + std::to_string(g_sigma[2])).c_str() : "");
    if (!dense.empty()) write_dense(dense, "filtered");
    apply_labels(ctx);
    apply_measure(ctx);
    apply_thickness(ctx);
    apply_geodesic(ctx);
    apply_skeleton(ctx);
    apply_diffusion(ctx);
}

// --tf PATH: the whole file as little-endian f32 RGBA rows (the library checks n, finiteness and alpha)
static std::vector<float> read_tf(const std::string &path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot open " + path);
    const std::streamsize bytes = f.tellg();
    if (bytes <= 0 || bytes % 16) throw std::runtime_error(path + ": expected whole RGBA rows of 4 f32 (16 bytes each)");
    std::vector<float> t((size_t)bytes / 4);
    f.seekg(0);
    f.read(reinterpret_cast<char *>(t.data()), bytes);
    if (f.gcount() != bytes) throw std::runtime_error(path + ": short read");
    return t;
}

// --auto-window, once the volume is there: the percentiles' window becomes the table's domain; without --tf the table is the grey ramp
static void apply_auto_window(Context &ctx) {
    const Histogram h = ctx.volume_histogram(VK_HIST_MAX_BINS, 0.0f, 1.0f);
    const std::pair<float, float> w = h.window(g_auto_lo, g_auto_hi);
    g_tf_lo = w.first; g_tf_hi = w.second;
    if (g_tf.empty()) g_tf = {0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
    std::printf("auto window: percentiles %g .. %g of %llu voxels -> [%g, %g]\n", g_auto_lo, g_auto_hi, (unsigned long long)h.stats.n_voxels, g_tf_lo, g_tf_hi);
    ctx.set_transfer_function(g_tf.data(), (uint32_t)(g_tf.size() / 4), g_tf_lo, g_tf_hi);
}

// --histogram in place of the raycast: the statistics in sample values, then `bin count` for every non-empty bin
static int run_histogram(uint32_t bins, float lo, float hi) {
    try {
        const HdrBackBuffer bb = pass_backbuffer();
        const Camera cam = pass_camera();
        Context ctx(bb.width, bb.height, &cam, 0, bb);
        if (g_clip_on) ctx.set_clip_box(&g_clip);
        if (!g_raw.empty()) VolumeTexture::from_raw(ctx, g_raw, g_dims[0], g_dims[1], g_dims[2], g_raw_fmt);
        else VolumeTexture::generate(ctx, VK_GEN_BONSAI_STANDIN, g_dims[0], g_dims[1], g_dims[2]);
        apply_filters(ctx);
        const Histogram h = ctx.volume_histogram(bins, lo, hi, nullptr, g_clip_on);
        const vk_volume_stats &s = h.stats;
        const double S = s.scale, n = (double)s.n_finite, mean = n > 0 ? s.sum / n : NAN, var = n > 0 ? std::max(s.sum_sq / n - mean * mean, 0.0) : NAN;
        std::printf("histogram: %u bins over [%g, %g], %llu voxels: %llu NaN, %llu below, %llu above\n", bins, lo, hi, (unsigned long long)s.n_voxels,
                    (unsigned long long)s.n_nan, (unsigned long long)s.n_below, (unsigned long long)s.n_above);
        std::printf("min %g max %g mean %g std %g (%llu finite)\n", s.min / S, s.max / S, mean / S, std::sqrt(var) / S, (unsigned long long)s.n_finite);
        for (uint32_t b = 0; b < bins; b++)
            if (h.counts[b]) std::printf("%u %llu\n", b, (unsigned long long)h.counts[b]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bonsai: %s\n", e.what());
        return 1;
    }
    return 0;
}

// --mesh in place of the raycast: the triangles as binary STL (facet normals formed in double) or as OBJ welded by bit pattern
static int run_mesh(const std::string &path, bool obj, float iso, const double scale[3]) {
    try {
        const HdrBackBuffer bb = pass_backbuffer();
        const Camera cam = pass_camera();
        Context ctx(bb.width, bb.height, &cam, 0, bb);
        if (g_clip_on) ctx.set_clip_box(&g_clip);
        if (!g_raw.empty()) VolumeTexture::from_raw(ctx, g_raw, g_dims[0], g_dims[1], g_dims[2], g_raw_fmt);
        else VolumeTexture::generate(ctx, VK_GEN_BONSAI_STANDIN, g_dims[0], g_dims[1], g_dims[2]);
        apply_filters(ctx);
        const std::vector<float> tris = ctx.extract_isosurface(iso, nullptr, g_clip_on);
        const size_t n = tris.size() / 9;
        if (!obj && n > 0xffffffffull) throw std::runtime_error("binary STL holds at most 2^32 - 1 triangles");
        std::ofstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("cannot open " + path);
        size_t n_vertices = 3 * n;
        if (obj) {
            std::map<std::array<uint32_t, 3>, uint32_t> seen;  // a vertex's bit pattern -> its 1-based index
            std::vector<uint32_t> faces(3 * n);
            char line[128];
            for (size_t v = 0; v < 3 * n; v++) {
                std::array<uint32_t, 3> key;
                std::memcpy(key.data(), &tris[3 * v], 12);
                auto it = seen.find(key);
                if (it == seen.end()) {
                    it = seen.emplace(key, (uint32_t)seen.size() + 1u).first;
                    const int len = std::snprintf(line, sizeof line, "v %.9g %.9g %.9g\n", tris[3 * v] * scale[0], tris[3 * v + 1] * scale[1], tris[3 * v + 2] * scale[2]);
                    f.write(line, len);
                }
                faces[v] = it->second;
            }
            for (size_t t = 0; t < n; t++) {
                const int len = std::snprintf(line, sizeof line, "f %u %u %u\n", faces[3 * t], faces[3 * t + 1], faces[3 * t + 2]);
                f.write(line, len);
            }
            n_vertices = seen.size();
        } else {
            char header[80];
            std::memset(header, ' ', sizeof header);
            std::memcpy(header, "vokselis_amd isosurface", 23);
            f.write(header, 80);
            const uint32_t n32 = (uint32_t)n;
            f.write(reinterpret_cast<const char *>(&n32), 4);
            for (size_t t = 0; t < n; t++) {
                double p[3][3];
                for (int v = 0; v < 3; v++)
                    for (int c = 0; c < 3; c++) p[v][c] = (double)tris[9 * t + 3 * v + c] * scale[c];
                const double a[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, b[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
                double nr[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
                const double len = std::sqrt(nr[0] * nr[0] + nr[1] * nr[1] + nr[2] * nr[2]);
                float rec[12];
                for (int c = 0; c < 3; c++) rec[c] = len > 0.0 ? (float)(nr[c] / len) : 0.0f;
                for (int v = 0; v < 3; v++)
                    for (int c = 0; c < 3; c++) rec[3 + 3 * v + c] = (float)p[v][c];
                const uint16_t attr = 0;
                f.write(reinterpret_cast<const char *>(rec), 48);
                f.write(reinterpret_cast<const char *>(&attr), 2);
            }
        }
        if (!f) throw std::runtime_error("cannot write " + path);
        std::printf("mesh: iso %g, %zu triangles, %zu vertices -> %s\n", iso, n, n_vertices, path.c_str());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bonsai: %s\n", e.what());
        return 1;
    }
    return 0;
}

struct Bonsai : Demo {
    std::unique_ptr<VolumeTexture> volume_texture;
    RaycastPipeline pipeline;
    static std::unique_ptr<Bonsai> init(Context &ctx) {  // examples/bonsai/main.rs:16-25
        auto self = std::make_unique<Bonsai>();
        if (!g_tf.empty() && !g_auto_window) ctx.set_transfer_function(g_tf.data(), (uint32_t)(g_tf.size() / 4), g_tf_lo, g_tf_hi);
        if (g_lit && !g_auto_window) ctx.set_lighting(&g_light);
        if (g_mip) ctx.set_projection(VK_PROJ_MAX);
        if (g_iso_on) ctx.set_isosurface(&g_iso);
        if (g_shadows_on) ctx.set_shadows(&g_shadows);
        if (g_clip_on) ctx.set_clip_box(&g_clip);
        if (!g_raw.empty()) self->volume_texture = std::make_unique<VolumeTexture>(VolumeTexture::from_raw(ctx, g_raw, g_dims[0], g_dims[1], g_dims[2], g_raw_fmt));
        else self->volume_texture = std::make_unique<VolumeTexture>(VolumeTexture::generate(ctx, VK_GEN_BONSAI_STANDIN, 256, 256, 256));
        apply_filters(ctx);
        if (g_auto_window) {  // the table follows the volume it is windowed to (and lighting its table)
            apply_auto_window(ctx);
            if (g_lit) ctx.set_lighting(&g_light);
        }
        self->pipeline = RaycastPipeline{VK_MODE_NAIVE_TRILINEAR, g_dt, 0};
        return self;
    }
    void update(Context &ctx) override { if (g_orbit) ctx.camera.add_yaw(6.28318f / 1024.f); }  // (a mouse drag: src/lib.rs:166-171)
    void render(Context &ctx) override { pipeline.record(ctx); }  // examples/bonsai/main.rs:27-57
};

// The frame's tiles over the node's GPUs (examples/xor/main.rs:235-254 generalised): one context per GPU inside a
// vk_group, the volume replicated, `batch` frames per launch / gather / un-tile.
static int run_group(int n_gpus, uint32_t frames, uint32_t batch, uint32_t w, uint32_t h, bool peer_direct) {
    std::vector<int> ords(n_gpus);
    for (int i = 0; i < n_gpus; i++) ords[i] = i;
    vk_group *g = nullptr;
    if (vk_group_create(n_gpus, ords.data(), &g) != VK_OK) { std::fprintf(stderr, "bonsai: vk_group_create: %s\n", vk_last_error(nullptr)); return 1; }
    int rc = 1;
    try {
        std::vector<char> raw;
        if (!g_raw.empty()) raw = VolumeTexture::read_raw(g_raw, g_dims[0], g_dims[1], g_dims[2], g_raw_fmt);
        for (int i = 0; i < n_gpus; i++) {
            vk_ctx *c = vk_group_ctx(g, i);
            check(c, vk_backbuffer_resize(c, w, h, VK_OUT_RGBA16F));
            if (!g_tf.empty()) check(c, vk_set_transfer_function(c, g_tf.data(), (uint32_t)(g_tf.size() / 4), g_tf_lo, g_tf_hi));
            if (g_lit) check(c, vk_set_lighting(c, &g_light));
            if (g_mip) check(c, vk_set_projection(c, VK_PROJ_MAX));
            if (g_iso_on) check(c, vk_set_isosurface(c, &g_iso));
            if (g_shadows_on) check(c, vk_set_shadows(c, &g_shadows));
            if (g_clip_on) check(c, vk_set_clip_box(c, &g_clip));
            if (!raw.empty()) check(c, vk_volume_upload(c, raw.data(), nullptr, g_dims[0], g_dims[1], g_dims[2], g_raw_fmt, VK_LAYOUT_AUTO));
            else check(c, vk_volume_generate(c, VK_GEN_BONSAI_STANDIN, 256, 256, 256, VK_FMT_R8_UNORM, 0x5EED0001u, 0, 1, VK_LAYOUT_AUTO));
        }
        vk_ctx *root = vk_group_ctx(g, 0);
        check(root, vk_partition_wire(root, VK_WIRE_RGB));  // tiles travel as colour only: alpha is 1 in every pixel (6 bytes instead of 8 per link and pixel)
        // --peer-direct: every GPU's march stores its tiles straight into GPU 0's frames over xGMI (no gather, no un-tile)
        if (peer_direct && vk_group_peer_direct(g, 1) != VK_OK) throw std::runtime_error(vk_group_last_error(g));
        Camera camera(1.f, 0.5f, 1.f, {0.5f, 0.5f, 0.5f}, (float)w / (float)h);
        // every frame of a launch its own camera: consecutive frames of an orbit (yaw step 2 pi / 1024), as bench.py's headline marches them
        std::vector<CameraUniform> cams;
        for (uint32_t j = 0; j < batch; j++) cams.push_back(Camera(1.f, 0.5f, 1.f + 6.28318f * (float)j / 1024.f, {0.5f, 0.5f, 0.5f}, (float)w / (float)h).get_proj_view_matrix());
        (void)camera;
        void *out = nullptr;
        check(root, vk_device_alloc(root, (size_t)batch * w * h * 8, &out));
        auto launch = [&]() { if (vk_group_render(g, VK_MODE_NAIVE_TRILINEAR, batch, cams.data(), 64, g_dt, 0, out) != VK_OK) throw std::runtime_error(vk_group_last_error(g)); };
        launch();
        if (vk_group_sync(g) != VK_OK) throw std::runtime_error(vk_group_last_error(g));
        const uint32_t n_batches = (frames + batch - 1) / batch;
        auto t0 = std::chrono::steady_clock::now();
        for (uint32_t b = 0; b < n_batches; b++) launch();
        if (vk_group_sync(g) != VK_OK) throw std::runtime_error(vk_group_last_error(g));
        double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / (n_batches * batch);
        std::vector<uint16_t> first((size_t)w * h * 4);
        check(root, vk_device_download(root, first.data(), out, first.size() * 2));
        uint64_t sum = 0;
        for (uint16_t v : first) sum += v;
        std::printf("tiles: %s\n", peer_direct ? "peer-direct stores into GPU 0's frames" : "gathered over RCCL, un-tiled on GPU 0");
        std::printf("GPUs %d, %u frames per launch\nAvg frame time %.4fms over %u frames\nframe 0 half-word sum %llu\n", n_gpus, batch, ms, n_batches * batch,
                    (unsigned long long)sum);
        check(root, vk_device_free(root, out));
        rc = 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bonsai: %s\n", e.what());
    }
    vk_group_destroy(g);
    return rc;
}

// --slice / --slice-plane: the plane's four vectors, formed in double and rounded once per component.  The volume's physical sides are its
// dims (unit spacing) over the longest of them; a pixel is `px` of that on both screen axes.
struct SliceArgs {
    bool on = false, oblique = false;
    int axis = 2;
    double pos = 0.5, centre[3] = {0.5, 0.5, 0.5}, normal[3] = {0.0, 0.0, 1.0}, extent = 1.0, thickness = 0.0;
    uint32_t samples = 1;
    int reduce = VK_SLAB_MAX;
};
static vk_slice make_slice(const SliceArgs &a, uint32_t w, uint32_t h) {
    const double longest = (double)std::max(g_dims[0], std::max(g_dims[1], g_dims[2]));
    const double size[3] = {g_dims[0] / longest, g_dims[1] / longest, g_dims[2] / longest};
    double n[3] = {0, 0, 0}, right[3] = {0, 0, 0}, down[3] = {0, 0, 0}, centre[3], px;  // unit directions in voxel space: the normal, +x and +y on screen
    if (a.oblique) {
        const double len = std::sqrt(a.normal[0] * a.normal[0] + a.normal[1] * a.normal[1] + a.normal[2] * a.normal[2]);
        for (int k = 0; k < 3; k++) { n[k] = a.normal[k] / len; centre[k] = a.centre[k]; }
        const int u = std::fabs(n[2]) < 0.9 ? 2 : 1;  // up: z, or y for a plane facing z; made perpendicular to the normal
        double up[3], ul = 0.0;
        for (int k = 0; k < 3; k++) { up[k] = (k == u ? 1.0 : 0.0) - n[u] * n[k]; ul += up[k] * up[k]; }
        for (int k = 0; k < 3; k++) { up[k] /= std::sqrt(ul); down[k] = 0.0 - up[k]; }
        right[0] = up[1] * n[2] - up[2] * n[1]; right[1] = up[2] * n[0] - up[0] * n[2]; right[2] = up[0] * n[1] - up[1] * n[0];  // up x normal
        px = a.extent / w;
    } else {
        const int sa = a.axis == 0 ? 1 : 0, sb = a.axis == 2 ? 1 : 2;  // the screen's axes run up the volume's: (x, y), (x, z), (y, z)
        n[a.axis] = 1.0; right[sa] = 1.0; down[sb] = 1.0;
        for (int k = 0; k < 3; k++) centre[k] = 0.5;
        centre[a.axis] = a.pos;
        px = std::max(size[sa] / w, size[sb] / h);  // the face fits the frame
    }
    vk_slice s{};
    const double step = a.samples > 1 ? a.thickness / (a.samples - 1) : 0.0;
    for (int k = 0; k < 3; k++) {
        const double du = right[k] * px / size[k], dv = down[k] * px / size[k];
        s.du[k] = (float)du; s.dv[k] = (float)dv; s.dn[k] = (float)(n[k] * step / size[k]);
        s.origin[k] = (float)(centre[k] - 0.5 * (w - 1) * du - 0.5 * (h - 1) * dv);
    }
    s.samples = a.samples;
    s.reduce = a.reduce;
    return s;
}

// The slice pass in place of the raycast: one pass with the value surface, the frame as a PPM (the stored sRGB, clamped to 0 .. 1).
static int run_slice(const SliceArgs &a, uint32_t w, uint32_t h, const std::string &ppm) {
    try {
        HdrBackBuffer bb; bb.width = w; bb.height = h; bb.format = VK_OUT_RGBA32F;
        const Camera cam = pass_camera();
        Context ctx(w, h, &cam, 0, bb);
        if (!g_tf.empty() && !g_auto_window) ctx.set_transfer_function(g_tf.data(), (uint32_t)(g_tf.size() / 4), g_tf_lo, g_tf_hi);
        if (g_clip_on) ctx.set_clip_box(&g_clip);
        if (!g_raw.empty()) VolumeTexture::from_raw(ctx, g_raw, g_dims[0], g_dims[1], g_dims[2], g_raw_fmt);
        else VolumeTexture::generate(ctx, VK_GEN_BONSAI_STANDIN, g_dims[0], g_dims[1], g_dims[2]);
        apply_filters(ctx);
        if (g_auto_window) apply_auto_window(ctx);
        const vk_slice s = make_slice(a, w, h);
        ctx.render_slice(s, true);
        const std::vector<float> val = ctx.read_slice_values();
        const std::vector<float> px = ctx.read_backbuffer_f32();
        size_t inside = 0;
        float lo = INFINITY, hi = -INFINITY;
        for (size_t q = 0; q < (size_t)w * h; q++)
            if (val[2 * q + 1] != 0.0f) { inside++; lo = std::min(lo, val[2 * q]); hi = std::max(hi, val[2 * q]); }
        const vk_slice_sample mid = ctx.slice_probe(s, w / 2, h / 2);
        std::printf("slice: %ux%u, %u sample%s, %zu pixels inside, values in [%g, %g]; centre pixel at %.6f %.6f %.6f: %s %g\n", w, h, a.samples, a.samples == 1 ? "" : "s",
                    inside, inside ? lo : 0.0f, inside ? hi : 0.0f, mid.pos[0], mid.pos[1], mid.pos[2], mid.inside ? "value" : "outside,", mid.value);
        if (!ppm.empty()) {
            std::ofstream f(ppm, std::ios::binary);
            f << "P6\n" << w << " " << h << "\n255\n";
            for (size_t q = 0; q < (size_t)w * h; q++) {
                char c[3];
                for (int k = 0; k < 3; k++) c[k] = (char)(unsigned char)(std::min(std::max(px[4 * q + k], 0.0f), 1.0f) * 255.0f + 0.5f);
                f.write(c, 3);
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bonsai: %s\n", e.what());
        return 1;
    }
    return 0;
}

// `zoom pitch yaw tx ty tz aspect` per line -> 144 bytes per line (no GPU involved)
static int dump_camera_blobs(const std::string &in, const std::string &out) {
    std::ifstream f(in);
    std::ofstream o(out, std::ios::binary);
    if (!f || !o) { std::fprintf(stderr, "bonsai: cannot open %s / %s\n", in.c_str(), out.c_str()); return 1; }
    float z, p, y, tx, ty, tz, a;
    while (f >> z >> p >> y >> tx >> ty >> tz >> a) {
        CameraUniform u = Camera(z, p, y, {tx, ty, tz}, a).get_proj_view_matrix();
        o.write(reinterpret_cast<const char *>(&u), sizeof u);
    }
    return 0;
}

int main(int argc, char **argv) {
    uint32_t frames = 100, w = 1280, h = 720, batch = 8, in_flight = 1;
    int gpus = 0;
    bool f32 = false, peer_direct = false, fuse_present = false, record = false;
    std::string ppm, dump_rgba, dump_steps, depth_ppm;
    bool pick = false;
    uint32_t pick_x = 0, pick_y = 0;
    SliceArgs sl;
    bool slab = false;
    bool hist = false;
    uint32_t hist_bins = 256;
    float hist_lo = 0.0f, hist_hi = 1.0f;
    std::string mesh_path;
    bool mesh_iso_on = false, mesh_obj = false;
    float mesh_iso = 0.0f;
    double mesh_scale[3] = {1.0, 1.0, 1.0};
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&]() -> const char * { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--frames") frames = (uint32_t)std::atoi(next());
        else if (a == "--size") { if (std::sscanf(next(), "%ux%u", &w, &h) != 2) { std::fprintf(stderr, "--size WxH\n"); return 2; } }
        else if (a == "--dt") g_dt = (float)std::atof(next());
        else if (a == "--raw") { g_raw = next(); g_raw_fmt = VK_FMT_R8_UNORM; }
        else if (a == "--raw-u16") { g_raw = next(); g_raw_fmt = VK_FMT_R16_UNORM; }
        else if (a == "--dims") { for (int k = 0; k < 3; k++) g_dims[k] = (uint32_t)std::max(0, std::atoi(next())); }
        else if (a == "--ppm") ppm = next();
        else if (a == "--f32") f32 = true;
        else if (a == "--pick") { pick = true; pick_x = (uint32_t)std::max(0, std::atoi(next())); pick_y = (uint32_t)std::max(0, std::atoi(next())); }
        else if (a == "--depth-ppm") depth_ppm = next();
        else if (a == "--dump-rgba") dump_rgba = next();
        else if (a == "--dump-steps") dump_steps = next();
        else if (a == "--gpus") gpus = std::atoi(next());
        else if (a == "--peer-direct") peer_direct = true;
        else if (a == "--in-flight") in_flight = (uint32_t)std::max(1, std::atoi(next()));
        else if (a == "--orbit") g_orbit = true;
        else if (a == "--fuse-present") fuse_present = true;
        else if (a == "--record") record = true;
        else if (a == "--batch") batch = (uint32_t)std::max(1, std::atoi(next()));
        else if (a == "--tf") {
            try { g_tf = read_tf(next()); } catch (const std::exception &e) { std::fprintf(stderr, "bonsai: %s\n", e.what()); return 1; }
        }
        else if (a == "--tf-domain") { g_tf_lo = (float)std::atof(next()); g_tf_hi = (float)std::atof(next()); }
        else if (a == "--mip") g_mip = true;
        else if (a == "--iso") { g_iso_on = true; g_iso.iso = (float)std::atof(next()); }
        else if (a == "--iso-colour") { for (int k = 0; k < 3; k++) g_iso.rgb[k] = (float)std::atof(next()); }
        else if (a == "--clip") { g_clip_on = true; for (int k = 0; k < 3; k++) g_clip.lo[k] = (float)std::atof(next()); for (int k = 0; k < 3; k++) g_clip.hi[k] = (float)std::atof(next()); }
        else if (a == "--shadows") { g_shadows_on = true; g_shadows.strength = (float)std::atof(next()); g_shadows.bias = (float)std::atof(next()); }
        else if (a == "--iso-refine") g_iso.refine = (uint32_t)std::max(0, std::atoi(next()));
        else if (a == "--light") { g_lit = true; g_light.headlight = 0; for (int k = 0; k < 3; k++) g_light.dir[k] = (float)std::atof(next()); }
        else if (a == "--headlight") { g_lit = true; g_light.headlight = 1; }
        else if (a == "--light-params") {
            g_light.ambient = (float)std::atof(next()); g_light.diffuse = (float)std::atof(next());
            g_light.specular = (float)std::atof(next()); g_light.shininess = (float)std::atof(next());
        }
        else if (a == "--slice") {
            const std::string ax = next();
            if (ax != "x" && ax != "y" && ax != "z") { std::fprintf(stderr, "bonsai: --slice AXIS POS: AXIS is x, y or z\n"); return 2; }
            if (sl.on) { std::fprintf(stderr, "bonsai: --slice and --slice-plane exclude each other (one plane per run)\n"); return 2; }
            sl.on = true; sl.oblique = false; sl.axis = ax[0] - 'x';
            sl.pos = std::atof(next());
            if (!(sl.pos >= 0.0 && sl.pos <= 1.0)) { std::fprintf(stderr, "bonsai: --slice AXIS POS: POS lies in 0 .. 1\n"); return 2; }
        }
        else if (a == "--slice-plane") {
            if (sl.on) { std::fprintf(stderr, "bonsai: --slice and --slice-plane exclude each other (one plane per run)\n"); return 2; }
            sl.on = true; sl.oblique = true;
            for (int k = 0; k < 3; k++) sl.centre[k] = std::atof(next());
            for (int k = 0; k < 3; k++) sl.normal[k] = std::atof(next());
            sl.extent = std::atof(next());
            const double len2 = sl.normal[0] * sl.normal[0] + sl.normal[1] * sl.normal[1] + sl.normal[2] * sl.normal[2];
            if (!(len2 > 0.0) || !std::isfinite(len2)) { std::fprintf(stderr, "bonsai: --slice-plane: the normal has no direction\n"); return 2; }
            if (!(sl.extent > 0.0) || !std::isfinite(sl.extent)) { std::fprintf(stderr, "bonsai: --slice-plane: EXTENT must be finite and > 0\n"); return 2; }
            for (int k = 0; k < 3; k++) if (!std::isfinite(sl.centre[k])) { std::fprintf(stderr, "bonsai: --slice-plane: the centre is not finite\n"); return 2; }
        }
        else if (a == "--slab") {
            slab = true;
            const int n = std::atoi(next());
            sl.thickness = std::atof(next());
            const std::string red = next();
            if (n < 1 || n > VK_SLICE_MAX_SAMPLES) { std::fprintf(stderr, "bonsai: --slab SAMPLES THICKNESS max|min|mean: SAMPLES lies in 1 .. %d\n", VK_SLICE_MAX_SAMPLES); return 2; }
            if (!(sl.thickness >= 0.0) || !std::isfinite(sl.thickness)) { std::fprintf(stderr, "bonsai: --slab: THICKNESS must be finite and >= 0\n"); return 2; }
            if (red != "max" && red != "min" && red != "mean") { std::fprintf(stderr, "bonsai: --slab: the reduction is max, min or mean\n"); return 2; }
            sl.samples = (uint32_t)n;
            sl.reduce = red == "max" ? VK_SLAB_MAX : (red == "min" ? VK_SLAB_MIN : VK_SLAB_MEAN);
        }
        else if (a == "--histogram") {
            hist = true;
            const int n = std::atoi(next());
            if (n < 1 || n > VK_HIST_MAX_BINS) { std::fprintf(stderr, "bonsai: --histogram BINS [LO HI]: BINS lies in 1 .. %d\n", VK_HIST_MAX_BINS); return 2; }
            hist_bins = (uint32_t)n;
            if (i + 2 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0 && std::string(argv[i + 2]).rfind("--", 0) != 0) { hist_lo = (float)std::atof(next()); hist_hi = (float)std::atof(next()); }
            else if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) { std::fprintf(stderr, "bonsai: --histogram BINS [LO HI]: LO needs HI\n"); return 2; }
            if (!std::isfinite(hist_lo) || !std::isfinite(hist_hi) || !(hist_hi > hist_lo)) { std::fprintf(stderr, "bonsai: --histogram BINS [LO HI]: LO and HI must be finite, LO < HI\n"); return 2; }
        }
        else if (a == "--mesh") {
            mesh_path = next();
            const std::string ext = mesh_path.size() >= 4 ? mesh_path.substr(mesh_path.size() - 4) : "";
            if (ext != ".stl" && ext != ".obj") { std::fprintf(stderr, "bonsai: --mesh OUT.stl|OUT.obj: the file name ends in .stl or .obj\n"); return 2; }
            mesh_obj = ext == ".obj";
        }
        else if (a == "--mesh-iso") {
            mesh_iso_on = true; mesh_iso = (float)std::atof(next());
            if (!std::isfinite(mesh_iso)) { std::fprintf(stderr, "bonsai: --mesh-iso V: V must be finite\n"); return 2; }
        }
        else if (a == "--mesh-scale") {
            for (int k = 0; k < 3; k++) mesh_scale[k] = std::atof(next());
            for (int k = 0; k < 3; k++) if (!(mesh_scale[k] > 0.0) || !std::isfinite(mesh_scale[k])) { std::fprintf(stderr, "bonsai: --mesh-scale SX SY SZ: finite and > 0\n"); return 2; }
        }
        else if (a == "--auto-window") {
            g_auto_window = true;
            g_auto_lo = std::atof(next()); g_auto_hi = std::atof(next());
            if (!(0.0 <= g_auto_lo && g_auto_lo < g_auto_hi && g_auto_hi <= 1.0)) { std::fprintf(stderr, "bonsai: --auto-window P_LO P_HI: needs 0 <= P_LO < P_HI <= 1\n"); return 2; }
        }
        else if (a == "--median") g_median = true;
        else if (a == "--smooth") {
            g_smooth = true;
            for (int k = 0; k < 3; k++) g_sigma[k] = std::atof(next());
            for (int k = 0; k < 3; k++) if (!(g_sigma[k] >= 0.0) || !std::isfinite(g_sigma[k])) { std::fprintf(stderr, "bonsai: --smooth SX SY SZ: finite and >= 0 (0: the axis is skipped)\n"); return 2; }
            if (g_sigma[0] == 0.0 && g_sigma[1] == 0.0 && g_sigma[2] == 0.0) { std::fprintf(stderr, "bonsai: --smooth SX SY SZ: at least one sigma above 0\n"); return 2; }
        }
        else if (a == "--save-raw") g_save_raw = next();
        else if (a == "--crop" || a == "--resample" || a == "--downsample" || a == "--isotropic" || a == "--to-u8" || a == "--to-u16") {
            ResampleOp op{};
            if (a == "--crop") {
                op.name = "crop";
                const std::string first = next();
                if (first == "clip") op.kind = ResampleOp::CROP_CLIP;
                else {
                    op.kind = ResampleOp::CROP;
                    long v[6];
                    v[0] = std::atol(first.c_str());
                    for (int k = 1; k < 6; k++) v[k] = std::atol(next());
                    for (int k = 0; k < 6; k++) if (v[k] < 0 || v[k] > 65535) { std::fprintf(stderr, "bonsai: --crop X0 Y0 Z0 X1 Y1 Z1: voxel indices of 0 .. 65535, or --crop clip\n"); return 2; }
                    if (v[0] >= v[3] || v[1] >= v[4] || v[2] >= v[5]) { std::fprintf(stderr, "bonsai: --crop X0 Y0 Z0 X1 Y1 Z1: a half-open box with X0 < X1, Y0 < Y1, Z0 < Z1\n"); return 2; }
                    op.box = vk_voxel_box{(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], (uint32_t)v[3], (uint32_t)v[4], (uint32_t)v[5]};
                }
            } else if (a == "--resample") {
                op.kind = ResampleOp::RESIZE; op.name = "resample"; op.mode = VK_RESAMPLE_LINEAR;
                for (int k = 0; k < 3; k++) {
                    const long v = std::atol(next());
                    if (v < 0 || v > 65535) { std::fprintf(stderr, "bonsai: --resample NX NY NZ: extents of 0 .. 65535 (0: the axis keeps its extent)\n"); return 2; }
                    op.dims[k] = (uint32_t)v;
                }
                if (i + 1 < argc && argv[i + 1][0] != '-') {
                    const std::string m = argv[++i];
                    if (m == "nearest") op.mode = VK_RESAMPLE_NEAREST; else if (m == "linear") op.mode = VK_RESAMPLE_LINEAR; else if (m == "area") op.mode = VK_RESAMPLE_AREA;
                    else { std::fprintf(stderr, "bonsai: --resample NX NY NZ [MODE]: MODE is nearest, linear or area\n"); return 2; }
                }
            } else if (a == "--downsample") {
                op.kind = ResampleOp::DOWNSAMPLE; op.name = "downsample";
                const long f = std::atol(next());
                if (f < 1 || f > VK_RESAMPLE_MAX_RATIO) { std::fprintf(stderr, "bonsai: --downsample F: an integer of 1 .. 16\n"); return 2; }
                op.dims[0] = (uint32_t)f;
            } else if (a == "--isotropic") {
                op.kind = ResampleOp::ISOTROPIC; op.name = "isotropic";
                for (int k = 0; k < 3; k++) {
                    op.spacing[k] = std::atof(next());
                    if (!std::isfinite(op.spacing[k]) || !(op.spacing[k] > 0.0)) { std::fprintf(stderr, "bonsai: --isotropic SX SY SZ: finite spacings above 0\n"); return 2; }
                }
            } else {
                op.kind = ResampleOp::CONVERT; op.name = a == "--to-u8" ? "to-u8" : "to-u16"; op.format = a == "--to-u8" ? VK_FMT_R8_UNORM : VK_FMT_R16_UNORM;
                for (int k = 0; k < 2; k++) op.window[k] = (float)std::atof(next());
                if (!std::isfinite(op.window[0]) || !std::isfinite(op.window[1]) || !(op.window[0] < op.window[1])) { std::fprintf(stderr, "bonsai: %s LO HI: finite sample values with LO < HI\n", a.c_str()); return 2; }
            }
            if (g_resample.size() >= 16u) { std::fprintf(stderr, "bonsai: --crop, --resample, --downsample, --isotropic, --to-u8 and --to-u16: at most 16 together\n"); return 2; }
            g_resample.push_back(op);
        }
        else if (a == "--components") {
            g_components = true;
            g_label_lo = (float)std::atof(next()); g_label_hi = (float)std::atof(next());
            if (std::isnan(g_label_lo) || std::isnan(g_label_hi) || g_label_lo > g_label_hi) { std::fprintf(stderr, "bonsai: --components LO HI [CONN]: needs LO <= HI, neither a NaN (HI may be inf)\n"); return 2; }
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) {
                const int c = std::atoi(next());
                if (c != 6 && c != 18 && c != 26) { std::fprintf(stderr, "bonsai: --components LO HI [CONN]: CONN is 6, 18 or 26\n"); return 2; }
                g_label_conn = (uint32_t)c;
                g_label_conn_on = true;
            }
        }
        else if (a == "--keep-largest" || a == "--drop-islands") {
            const long long n = std::atoll(next());
            if (n < 1) { std::fprintf(stderr, "bonsai: %s: a count of at least 1\n", a.c_str()); return 2; }
            std::vector<uint64_t> &list = a == "--keep-largest" ? g_keep_largest : g_drop_islands;
            if (list.size() >= 16u) { std::fprintf(stderr, "bonsai: %s: at most 16 times\n", a.c_str()); return 2; }
            list.push_back((uint64_t)n);
        }
        else if (a == "--keep-voxel" || a == "--remove-voxel") {
            std::array<uint32_t, 3> v{};
            for (int k = 0; k < 3; k++) { const long long c = std::atoll(next()); if (c < 0 || c > 0xffffffffll) { std::fprintf(stderr, "bonsai: %s X Y Z: voxel indices >= 0\n", a.c_str()); return 2; } v[k] = (uint32_t)c; }
            std::vector<std::array<uint32_t, 3>> &list = a == "--keep-voxel" ? g_keep_voxels : g_remove_voxels;
            if (list.size() >= 16u) { std::fprintf(stderr, "bonsai: %s: at most 16 times\n", a.c_str()); return 2; }
            list.push_back(v);
        }
        else if (a == "--keep-pick") {
            std::array<uint32_t, 2> p{};
            for (int k = 0; k < 2; k++) p[k] = (uint32_t)std::max(0, std::atoi(next()));
            if (g_keep_picks.size() >= 16u) { std::fprintf(stderr, "bonsai: --keep-pick: at most 16 times\n"); return 2; }
            g_keep_picks.push_back(p);
        }
        else if (a == "--label-fill") {
            g_label_fill_on = true; g_label_fill = (float)std::atof(next());
            if (!std::isfinite(g_label_fill)) { std::fprintf(stderr, "bonsai: --label-fill V: V must be finite\n"); return 2; }
        }
        else if (a == "--morph") {
            const std::string name = next();
            const float radius = (float)std::atof(next());
            static const struct { const char *name; int op; } known[] = {{"close", VK_DIST_CLOSE}, {"open", VK_DIST_OPEN}, {"dilate", VK_DIST_DILATE}, {"erode", VK_DIST_ERODE}};
            const auto *found = std::find_if(std::begin(known), std::end(known), [&](const auto &k) { return name == k.name; });
            if (found == std::end(known)) { std::fprintf(stderr, "bonsai: --morph OP RADIUS: OP is close, open, dilate or erode\n"); return 2; }
            if (!std::isfinite(radius) || radius < 0.0f || radius > VK_DIST_MAX_RADIUS) { std::fprintf(stderr, "bonsai: --morph OP RADIUS: a finite RADIUS of 0 .. 65535\n"); return 2; }
            if (g_morph.size() >= 16u) { std::fprintf(stderr, "bonsai: --morph: at most 16 times\n"); return 2; }
            g_morph.push_back({found->op, found->name, radius});
        }
        else if (a == "--split") {
            g_split_on = true;
            g_split_radius = (float)std::atof(next());
            if (!std::isfinite(g_split_radius) || g_split_radius < 0.0f || g_split_radius > VK_DIST_MAX_RADIUS) { std::fprintf(stderr, "bonsai: --split RADIUS [CONN]: a finite RADIUS of 0 .. 65535\n"); return 2; }
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) {
                const int c = std::atoi(next());
                if (c != 6 && c != 18 && c != 26) { std::fprintf(stderr, "bonsai: --split RADIUS [CONN]: CONN is 6, 18 or 26\n"); return 2; }
                g_split_conn = (uint32_t)c;
            }
        }
        else if (a == "--thickness") {
            if (g_thick_on) { std::fprintf(stderr, "bonsai: --thickness: at most once\n"); return 2; }
            g_thick_on = true;
            g_thick_radius = (float)std::atof(next());
            if (!std::isfinite(g_thick_radius) || g_thick_radius < 1.0f) { std::fprintf(stderr, "bonsai: --thickness MAX_RADIUS [GAIN]: a finite MAX_RADIUS of at least 1\n"); return 2; }
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) {
                g_thick_gain = (float)std::atof(next());
                if (!std::isfinite(g_thick_gain) || !(g_thick_gain > 0.0f)) { std::fprintf(stderr, "bonsai: --thickness MAX_RADIUS [GAIN]: a finite GAIN above 0\n"); return 2; }
            }
        }
        else if (a == "--geodesic") {
            if (g_geo_face_on) { std::fprintf(stderr, "bonsai: --geodesic: at most once\n"); return 2; }
            g_geo_on = g_geo_face_on = true;
            auto face = [&](const char *v, int &axis) -> uint32_t {
                static const char *const names[6] = {"x-", "x+", "y-", "y+", "z-", "z+"};
                for (int f = 0; f < 6; f++) if (std::string(v) == names[f]) { axis = f / 2; return 1u << f; }
                return 0u;
            };
            int axis = 0;
            g_geo_sources = face(next(), axis);
            if (!g_geo_sources) { std::fprintf(stderr, "bonsai: --geodesic FACE [TARGET_FACE]: a face is one of x- x+ y- y+ z- z+\n"); return 2; }
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) {
                g_geo_targets = face(next(), g_geo_axis);
                if (!g_geo_targets) { std::fprintf(stderr, "bonsai: --geodesic FACE [TARGET_FACE]: a face is one of x- x+ y- y+ z- z+\n"); return 2; }
            }
        }
        else if (a == "--geodesic-voxel") {
            g_geo_on = true;
            long long v[3];
            for (int c = 0; c < 3; c++) v[c] = std::atoll(next());
            if (v[0] < 0 || v[1] < 0 || v[2] < 0 || v[0] > 0xffffffffll || v[1] > 0xffffffffll || v[2] > 0xffffffffll) { std::fprintf(stderr, "bonsai: --geodesic-voxel X Y Z: three voxel indices >= 0\n"); return 2; }
            if (g_geo_seeds.size() >= (size_t)VK_GEO_MAX_SEEDS) { std::fprintf(stderr, "bonsai: --geodesic-voxel: at most 16 seeds\n"); return 2; }
            g_geo_seeds.push_back({(uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]});
        }
        else if (a == "--skeleton") {
            if (g_skel_on) { std::fprintf(stderr, "bonsai: --skeleton: at most once\n"); return 2; }
            g_skel_on = true;
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0 && !std::isdigit((unsigned char)argv[i + 1][0]) && argv[i + 1][0] != '-') {
                const std::string mode = next();
                if (mode == "kernel") g_skel_mode = VK_SKEL_KERNEL;
                else if (mode != "curve") { std::fprintf(stderr, "bonsai: --skeleton [curve|kernel] [MAX_ITER]: the mode is curve or kernel\n"); return 2; }
            }
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) {
                const char *v = next();
                char *end = nullptr;
                const long long k = std::strtoll(v, &end, 10);
                if (end == v || *end != '\0' || k < 0 || k > 0xffffffffll) { std::fprintf(stderr, "bonsai: --skeleton [curve|kernel] [MAX_ITER]: MAX_ITER is an integer >= 0\n"); return 2; }
                g_skel_max_iter = (uint32_t)k;
            }
        }
        else if (a == "--diffusion") {
            if (g_diff_on) { std::fprintf(stderr, "bonsai: --diffusion: at most once\n"); return 2; }
            g_diff_on = true;
            const std::string axis = next();
            if (axis != "x" && axis != "y" && axis != "z") { std::fprintf(stderr, "bonsai: --diffusion AXIS [MAX_SWEEPS]: AXIS is x, y or z\n"); return 2; }
            g_diff_axis = (uint32_t)(axis[0] - 'x');
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) {
                const char *v = next();
                char *end = nullptr;
                const long long k = std::strtoll(v, &end, 10);
                if (end == v || *end != '\0' || k < 32 || k > 0xffffffffll) { std::fprintf(stderr, "bonsai: --diffusion AXIS [MAX_SWEEPS]: MAX_SWEEPS is an integer >= 32 (a block of sweeps)\n"); return 2; }
                g_diff_max_sweeps = (uint32_t)k;
            }
        }
        else if (a == "--diffusion-install") g_diff_install = true;
        else if (a == "--measure") {
            g_measure_on = true;
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) g_measure_csv = next();
        }
        else if (a == "--morph-spacing") {
            g_morph_spacing_on = true;
            for (int k = 0; k < 3; k++) {
                const long long v = std::atoll(next());
                if (v < 1 || v > VK_DIST_MAX_SPACING) { std::fprintf(stderr, "bonsai: --morph-spacing SX SY SZ: integers of 1 .. 64\n"); return 2; }
                g_morph_spacing[k] = (uint32_t)v;
            }
        }
        else if (a == "--morph-fill") {
            g_morph_fill_on = true;
            for (int k = 0; k < 2; k++) g_morph_fill[k] = (float)std::atof(next());
            if (!std::isfinite(g_morph_fill[0]) || !std::isfinite(g_morph_fill[1])) { std::fprintf(stderr, "bonsai: --morph-fill IN OUT: finite values\n"); return 2; }
        }
        else if (a == "--camera-blobs") { std::string in = next(); return dump_camera_blobs(in, next()); }
        else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (g_iso_on && g_mip) { std::fprintf(stderr, "bonsai: --iso and --mip exclude each other (an isosurface ignores the projection)\n"); return 2; }
    if (g_shadows_on && !(g_iso_on && g_lit && !g_light.headlight)) { std::fprintf(stderr, "bonsai: --shadows needs --iso and --light (shadows are cast along a light direction, under an isosurface)\n"); return 2; }
    bool crop_clip = false;  // --crop clip consumes the box: nothing marches under it afterwards
    for (const ResampleOp &op : g_resample) crop_clip = crop_clip || op.kind == ResampleOp::CROP_CLIP;
    if (g_clip_on && !crop_clip && g_tf.empty() && !g_mip && !g_iso_on && !sl.on && !hist && mesh_path.empty()) { std::fprintf(stderr, "bonsai: --clip needs --tf, --mip or --iso (the built-in march has no clip kernels)\n"); return 2; }
    if ((pick || !depth_ppm.empty()) && !g_iso_on) { std::fprintf(stderr, "bonsai: --pick and --depth-ppm need --iso (the geometry pass is the isosurface's)\n"); return 2; }
    if (slab && !sl.on) { std::fprintf(stderr, "bonsai: --slab needs --slice or --slice-plane (a slab is a thick slice)\n"); return 2; }
    if (sl.on && gpus > 0) { std::fprintf(stderr, "bonsai: --slice and --slice-plane render on one GPU (groups have no slice output)\n"); return 2; }
    if (sl.on && (pick || !depth_ppm.empty() || !dump_rgba.empty() || !dump_steps.empty())) { std::fprintf(stderr, "bonsai: --slice and --slice-plane replace the raycast: no --pick, --depth-ppm, --dump-rgba or --dump-steps\n"); return 2; }
    if (hist && (sl.on || gpus > 0 || g_auto_window)) { std::fprintf(stderr, "bonsai: --histogram replaces the render: no --slice, --slice-plane, --gpus or --auto-window\n"); return 2; }
    if (g_auto_window && g_tf.empty() && !g_mip && !sl.on) { std::fprintf(stderr, "bonsai: --auto-window needs a mode that has a window: --tf, --mip, --slice or --slice-plane\n"); return 2; }
    if (g_auto_window && g_iso_on) { std::fprintf(stderr, "bonsai: --auto-window sets a table's domain: an isosurface (--iso) has none\n"); return 2; }
    if (g_auto_window && gpus > 0) { std::fprintf(stderr, "bonsai: --auto-window runs on one GPU\n"); return 2; }
    if (mesh_path.empty() && (mesh_iso_on || mesh_scale[0] != 1.0 || mesh_scale[1] != 1.0 || mesh_scale[2] != 1.0)) { std::fprintf(stderr, "bonsai: --mesh-iso and --mesh-scale need --mesh\n"); return 2; }
    if (!mesh_path.empty() && !mesh_iso_on && !g_iso_on) { std::fprintf(stderr, "bonsai: --mesh needs an isovalue: --mesh-iso V or --iso V\n"); return 2; }
    if (!mesh_path.empty() && !mesh_iso_on && !std::isfinite(g_iso.iso)) { std::fprintf(stderr, "bonsai: --mesh: the isovalue must be finite\n"); return 2; }
    if (!mesh_path.empty() && (sl.on || hist || gpus > 0 || g_auto_window)) { std::fprintf(stderr, "bonsai: --mesh replaces the render: no --slice, --slice-plane, --histogram, --gpus or --auto-window\n"); return 2; }
    if (label_ops() && !g_components && !g_iso_on) { std::fprintf(stderr, "bonsai: --keep-largest, --drop-islands, --keep-voxel, --remove-voxel and --keep-pick need a value range: --components LO HI, or --iso V for [V, inf)\n"); return 2; }
    if (!g_keep_picks.empty() && !g_iso_on) { std::fprintf(stderr, "bonsai: --keep-pick needs --iso (the ray stops at the isosurface)\n"); return 2; }
    if (g_label_fill_on && !label_ops() && !g_split_on && !g_thick_on && !g_geo_on && !g_skel_on && !(g_diff_on && g_diff_install)) { std::fprintf(stderr, "bonsai: --label-fill needs a flag that drops voxels: --keep-largest, --drop-islands, --keep-voxel, --remove-voxel or --keep-pick\n"); return 2; }
    if (g_keep_voxels.size() + g_keep_picks.size() > 16u) { std::fprintf(stderr, "bonsai: --keep-voxel and --keep-pick: at most 16 seeds together\n"); return 2; }
    if ((g_components || label_ops()) && gpus > 0) { std::fprintf(stderr, "bonsai: --components and the keep flags run on one GPU\n"); return 2; }
    if (!g_morph.empty() && !g_components && !g_iso_on) { std::fprintf(stderr, "bonsai: --morph needs a value range: --components LO HI, or --iso V for [V, inf)\n"); return 2; }
    if (g_split_on && !g_components && !g_iso_on) { std::fprintf(stderr, "bonsai: --split needs a value range: --components LO HI, or --iso V for [V, inf)\n"); return 2; }
    if (g_split_on && gpus > 0) { std::fprintf(stderr, "bonsai: --split runs on one GPU\n"); return 2; }
    if (g_measure_on && !g_components && !g_iso_on) { std::fprintf(stderr, "bonsai: --measure needs a value range: --components LO HI, or --iso V for [V, inf)\n"); return 2; }
    if (g_measure_on && gpus > 0) { std::fprintf(stderr, "bonsai: --measure runs on one GPU\n"); return 2; }
    if (g_thick_on && !g_components && !g_iso_on) { std::fprintf(stderr, "bonsai: --thickness needs a value range: --components LO HI, or --iso V for [V, inf)\n"); return 2; }
    if (g_thick_on && g_thick_radius / (float)std::min({g_morph_spacing[0], g_morph_spacing[1], g_morph_spacing[2]}) > (float)VK_THICK_MAX_REACH) {
        std::fprintf(stderr, "bonsai: --thickness MAX_RADIUS [GAIN]: MAX_RADIUS reaches further than 32 voxels of the smallest spacing\n"); return 2;
    }
    if (g_thick_on && gpus > 0) { std::fprintf(stderr, "bonsai: --thickness runs on one GPU\n"); return 2; }
    if (g_geo_on && !g_components && !g_iso_on) { std::fprintf(stderr, "bonsai: --geodesic and --geodesic-voxel need a value range: --components LO HI, or --iso V for [V, inf)\n"); return 2; }
    if (g_geo_on && gpus > 0) { std::fprintf(stderr, "bonsai: --geodesic runs on one GPU\n"); return 2; }
    if (g_skel_on && !g_components && !g_iso_on) { std::fprintf(stderr, "bonsai: --skeleton needs a value range: --components LO HI, or --iso V for [V, inf)\n"); return 2; }
    if (g_skel_on && gpus > 0) { std::fprintf(stderr, "bonsai: --skeleton runs on one GPU\n"); return 2; }
    if (g_diff_install && !g_diff_on) { std::fprintf(stderr, "bonsai: --diffusion-install needs --diffusion AXIS\n"); return 2; }
    if (g_diff_on && !g_components && !g_iso_on) { std::fprintf(stderr, "bonsai: --diffusion needs a value range: --components LO HI, or --iso V for [V, inf)\n"); return 2; }
    if (g_diff_on && gpus > 0) { std::fprintf(stderr, "bonsai: --diffusion runs on one GPU\n"); return 2; }
    g_diff_save = g_diff_on && g_diff_install && !g_save_raw.empty();
    if (((g_morph_spacing_on && !g_split_on && !g_measure_on && !g_thick_on && !g_geo_on && !g_skel_on && !g_diff_on) || g_morph_fill_on) && g_morph.empty()) { std::fprintf(stderr, "bonsai: %s needs --morph\n", g_morph_spacing_on ? "--morph-spacing" : "--morph-fill"); return 2; }
    if (!g_morph.empty() && gpus > 0) { std::fprintf(stderr, "bonsai: --morph runs on one GPU\n"); return 2; }
    if ((label_ops() || !g_morph.empty() || g_split_on || g_measure_on || g_thick_on || g_geo_on || g_skel_on || g_diff_on) && !g_components) { g_label_lo = g_iso.iso; g_label_hi = INFINITY; g_label_conn = 6; }
    g_w = w; g_h = h;
    if (!g_resample.empty() && gpus > 0) { std::fprintf(stderr, "bonsai: --crop, --resample, --downsample, --isotropic, --to-u8 and --to-u16 run on one GPU\n"); return 2; }
    for (const ResampleOp &op : g_resample)
        if (op.kind == ResampleOp::CROP_CLIP && !g_clip_on) { std::fprintf(stderr, "bonsai: --crop clip needs --clip\n"); return 2; }
    if (!g_save_raw.empty() && !g_median && !g_smooth && !label_ops() && g_morph.empty() && g_resample.empty() && !g_split_on && !g_thick_on && !g_geo_on && !g_skel_on && !g_diff_save) { std::fprintf(stderr, "bonsai: --save-raw writes the filtered volume: it needs --median or --smooth\n"); return 2; }
    if ((g_median || g_smooth) && gpus > 0) { std::fprintf(stderr, "bonsai: --median and --smooth run on one GPU\n"); return 2; }
    if (hist) return run_histogram(hist_bins, hist_lo, hist_hi);
    if (!mesh_path.empty()) return run_mesh(mesh_path, mesh_obj, mesh_iso_on ? mesh_iso : g_iso.iso, mesh_scale);
    if (sl.on) return run_slice(sl, w, h, ppm);
    if (gpus > 0) return run_group(gpus, frames, batch, w, h, peer_direct);
    try {
        // examples/bonsai/main.rs:64-74: 1280x720 window, Camera::new(1., 0.5, 1., (0.5,0.5,0.5), w/h)
        Camera camera(1.f, 0.5f, 1.f, {0.5f, 0.5f, 0.5f}, (float)w / (float)h);
        HdrBackBuffer bb; bb.width = w; bb.height = h;
        if (f32) bb.format = VK_OUT_RGBA32F;
        Context ctx(w, h, &camera, 0, bb);
        ctx.fuse_present = fuse_present;  // (the present pass in the raycast pass's epilogue: VK_RENDER_PRESENT)
        std::printf("%s\n", ctx.get_info().c_str());
        double ms = 0;
        // --record: the reference's recorder takes capture_frame() of every frame (src/lib.rs:196-199); with frames in flight it takes the frame
        // K - 1 ids back -- finished or nearly so -- while the newer ones execute
        std::vector<uint8_t> rec;
        uint64_t recorded = 0, rec_sum = 0;
        auto recorder = [&](Context &c, uint64_t id) {
            if (!record || id < in_flight) return;
            c.capture_frame_into(id - (in_flight - 1), rec);
            recorded++;
            rec_sum += rec[rec.size() / 2];
        };
        auto demo = run_headless<Bonsai>(ctx, frames, &ms, in_flight, recorder);
        std::printf("Avg frame time %.4fms over %u frames (%u in flight)\n", ms, frames, in_flight);  // src/utils/frame_counter.rs:23-24
        if (record) std::printf("recorded %llu frames (probe byte sum %llu)\n", (unsigned long long)recorded, (unsigned long long)rec_sum);
        auto shot = ctx.capture_frame();
        uint64_t sum = 0;
        for (uint8_t b : shot.first) sum += b;
        std::printf("capture_frame: %ux%u, padded row %u B, byte sum %llu\n", shot.second.width, shot.second.height,
                    shot.second.padded_bytes_per_row, (unsigned long long)sum);
        if (!dump_rgba.empty() || !dump_steps.empty()) {
            // the hot path's own output (before the present pass), with the kernel's per-pixel trip counts
            RaycastPipeline counted = demo->pipeline;
            counted.flags |= VK_RENDER_COUNT;
            counted.record(ctx);
            if (!dump_rgba.empty()) {
                std::vector<float> px = ctx.read_backbuffer_f32();
                std::ofstream(dump_rgba, std::ios::binary).write(reinterpret_cast<const char *>(px.data()), (std::streamsize)(px.size() * 4));
            }
            if (!dump_steps.empty()) {
                std::vector<uint32_t> st((size_t)w * h);
                check(ctx.handle(), vk_readback_steps(ctx.handle(), st.data()));
                std::ofstream(dump_steps, std::ios::binary).write(reinterpret_cast<const char *>(st.data()), (std::streamsize)(st.size() * 4));
            }
        }
        if (pick) {
            const vk_hit hit = ctx.pick(pick_x, pick_y, g_dt);
            if (!hit.hit) std::printf("pick (%u, %u): miss\n", pick_x, pick_y);
            else {
                const double g[3] = {hit.grad[0], hit.grad[1], hit.grad[2]}, len = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
                std::printf("pick (%u, %u): pos %.6f %.6f %.6f  t %.6f  value %g  grad %g %g %g", pick_x, pick_y, hit.pos[0], hit.pos[1], hit.pos[2], hit.t, hit.value,
                            hit.grad[0], hit.grad[1], hit.grad[2]);
                if (len > 0.0 && std::isfinite(len)) std::printf("  normal %.6f %.6f %.6f\n", -g[0] / len, -g[1] / len, -g[2] / len);
                else std::printf("  normal none (no gradient)\n");
            }
        }
        if (!depth_ppm.empty()) {
            ctx.render_geometry(g_dt);
            const std::vector<float> rec = ctx.read_geometry();
            float t_min = INFINITY, t_max = -INFINITY;
            size_t hits = 0;
            for (size_t q = 0; q < (size_t)w * h; q++) {
                const float t = rec[8 * q + 3];
                if (std::isfinite(t)) { t_min = std::min(t_min, t); t_max = std::max(t_max, t); hits++; }
            }
            std::ofstream f(depth_ppm, std::ios::binary);
            f << "P6\n" << w << " " << h << "\n255\n";
            for (size_t q = 0; q < (size_t)w * h; q++) {
                const float t = rec[8 * q + 3];
                unsigned char v = 0;  // a miss
                if (std::isfinite(t)) v = (unsigned char)(255.0f - 191.0f * (t_max > t_min ? (t - t_min) / (t_max - t_min) : 0.0f) + 0.5f);  // near 255 .. far 64
                const char px[3] = {(char)v, (char)v, (char)v};
                f.write(px, 3);
            }
            std::printf("depth: %zu hit pixels, t in [%g, %g] -> %s\n", hits, hits ? t_min : 0.0f, hits ? t_max : 0.0f, depth_ppm.c_str());
        }
        if (!ppm.empty()) {
            std::ofstream f(ppm, std::ios::binary);
            f << "P6\n" << shot.second.width << " " << shot.second.height << "\n255\n";
            for (uint32_t y = 0; y < shot.second.height; y++)
                for (uint32_t x = 0; x < shot.second.width; x++)
                    f.write((const char *)&shot.first[(size_t)y * shot.second.padded_bytes_per_row + x * 4], 3);
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "bonsai: %s\n", e.what());
        return 1;
    }
    return 0;
}
