/*
 * vokselis_hip.h -- C-ABI of the MI355X-native vokselis raycast path.
 *
 * The reference (pudnax/vokselis) has no FFI: its hot path sits behind the wgpu bind-group
 * contract of shaders/raycast_naive.wgsl and shaders/raycast_compute.wgsl, driven from
 * `Demo::render(&mut self, &Context)` (src/lib.rs:42,178-181).  Each entry point below replaces
 * one wgpu-side step of that contract; the reference lines it replaces are cited per function.
 * INTEGRATION.md shows the `extern "C"` block a Rust maintainer would add to bind it.
 *
 * Conventions: 0 = VK_OK, negative = error, nothing aborts or throws across the boundary.
 * The caller owns every host pointer; the library owns all device memory it allocates.  A
 * vk_ctx is bound to one GPU and one HIP stream (one per frame slot with frames in flight) and is
 * not thread-safe (the reference drives its queue from the single winit thread, src/lib.rs:71).
 */
#ifndef VOKSELIS_HIP_H
#define VOKSELIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VK_ABI_VERSION 5

typedef struct vk_ctx vk_ctx;

enum vk_status {
    VK_OK = 0,
    VK_ERR_INVALID = -1,   /* bad argument / wrong state */
    VK_ERR_HIP = -2,       /* a HIP runtime call failed; see vk_last_error */
    VK_ERR_NO_DEVICE = -3, /* no usable gfx950 device */
    VK_ERR_OOM = -4,
    VK_ERR_UNSUPPORTED = -5
};

/* src/context/volume_texture.rs:39-47 (R8Unorm), SURVEY C4 (R16Float),
 * examples/xor/xor_compute.rs:94-118 (two rgba16float storage textures).
 * R16_UNORM (wgpu's R16Unorm): `host` is the dense x-fastest array of native-endian uint16_t, the shader-side value
 * of a tap t is t / 65535, and the kernels filter the integer taps (S = 65535; every u16 is exact in f32) -- the 12- and 16-bit data
 * of CT / MR scans, which R8 requantises and R16F holds exactly only up to 2048.  NAIVE_TRILINEAR only, every family (built-in, table,
 * lit, MAX, isosurface, clip box); layouts LINEAR and PACKED (AUTO: PACKED wherever an R16F volume of the dimensions gets PACKED,
 * LINEAR where that volume would be STAGED); PACKED_PAIRS / BRICKED / QUADS / STAGED, vk_volume_generate and VK_RENDER_FAST_WALK are
 * VK_ERR_UNSUPPORTED with it. */
enum vk_volume_format { VK_FMT_R8_UNORM = 0, VK_FMT_R16_FLOAT = 1, VK_FMT_RGBA16F_PAIR = 2, VK_FMT_R16_UNORM = 3 };

/* raycast_naive.wgsl fs_main vs raycast_compute.wgsl render()/get_col2 */
enum vk_mode {
    VK_MODE_NAIVE_TRILINEAR = 0,
    VK_MODE_COMPUTE_NEAREST = 1,
    /* SURVEY 8(d) C3, "procedural, no volume texture": the reference has no such example (examples/trig draws one
     * triangle); this build defines it as the compute twin's ray and march (raycast_compute.wgsl:62-131) with the
     * texel loads replaced by the xor example's density function noise_volume(p / 2) (shaders/xor.wgsl:55-61,
     * un.time = the uploaded Uniform's time), colour = density.rgb / 2, no normals.  Needs no volume. */
    VK_MODE_PROCEDURAL = 2
};

/* src/context/hdr_backbuffer.rs:10 is rgba16float; RGBA32F is the parity surface. */
enum vk_out_format { VK_OUT_RGBA32F = 0, VK_OUT_RGBA16F = 1 };

/* How the library lays the scalar volume out in HBM (DESIGN.md "Data layout"). */
enum vk_layout {
    VK_LAYOUT_AUTO = 0,
    VK_LAYOUT_LINEAR = 1, /* x-fastest as uploaded; 8 scalar taps per sample (validation kernel) */
    VK_LAYOUT_PACKED = 2, /* 4^3-bricked cells, each holding its 8 trilinear taps (+ per-octant skip maps) */
    VK_LAYOUT_PACKED_PAIRS = 3, /* u8 volumes: cells hold 4 (tap, x-delta) f16 pairs, 16 B */
    VK_LAYOUT_BRICKED = 4, /* dense 8^3 bricks + 1-voxel apron (9^3): 1.42x the dense bytes, 8 taps from one
                              brick as four x-pair loads; the most compact layout (no skip map) */
    VK_LAYOUT_QUADS = 5, /* every element holds a voxel's 2x2 (y,z) neighbourhood: 8 taps = two consecutive elements
                           = ONE 8/16-byte load; 4.5x the dense bytes; pays when the image has more rays than the volume has
                           voxel columns (no skip map; never AUTO's choice) */
    VK_LAYOUT_STAGED = 6 /* dense 8^3 bricks (no apron; one copy per major ray axis) that every wave stages through LDS with
                            coalesced 16-byte LDS-DMA loads, taps read with ds_read: the layout for volumes far larger than
                            the caches (AUTO's choice above 4 GiB of cells; no skip map) */
};

enum vk_render_flags {
    VK_RENDER_NO_SKIP = 1,  /* disable exact empty-space skipping (every step fetches taps) */
    VK_RENDER_COUNT = 2,    /* also accumulate step counters / per-pixel step counts */
    VK_RENDER_SAFE = 4,     /* force the clamped / 64-bit-offset kernel variant */
    VK_RENDER_FORCE_SKIP = 8, /* use the skip kernel (with adaptive probing) whatever the census of transparent cells (default policy:
                                 dense kernel below 45 % of exactly transparent cells, adaptive probing from 45 %, probing on every trip from 55 %) */
    VK_RENDER_DEBUG_TRIPS = 16, /* with COUNT: vk_readback_steps returns march-loop trips (lookups) per pixel */
    VK_RENDER_DEBUG_FALLBACK = 32, /* with COUNT, VK_LAYOUT_STAGED: vk_readback_steps returns the steps whose taps came from global memory */
    VK_RENDER_PROBE_ALWAYS = 64, /* skip kernels: look the distance map up on every trip (no adaptive dense stretches): S_sampled is then
                                   exactly the number of steps that can contribute; the frame is the same either way */
    VK_RENDER_FAST_WALK = 128, /* TOLERANCE MODE of the skip kernels: a run of exactly transparent steps advances the ray in closed form
                                 (one fma per accumulator) instead of by the reference loop's own sequence of rounded additions
                                 (raycast_naive.wgsl:101,118).  t stays exact; the sample positions part from the default, bit-exact mode's
                                 by ~2e-4 cell where a coordinate crosses a power of two inside a skipped run: 99.99 % of C2's pixels
                                 within 1.04e-4, a handful per frame (0.004 %) whose alpha >= 0.95 early-out flips up to 2e-2 off.
                                 19 % faster on C2.  Ignored by kernels that do not skip. */
    /* ABI 5 -- the present pass fused into the raycast pass's epilogue (vk_render only).  When the window has the backbuffer's size,
     * Context::render's present (src/context.rs:251-297, shaders/present.wgsl:111-119) reads each texel once, at its centre: the
     * lane that holds the finished pixel applies ACESFilm + linear_to_srgb itself and writes the context's Rgba8Unorm target (what
     * vk_capture_frame reads) -- no second launch, and the 8-16 bytes per pixel the present pass would read back are never
     * fetched.  A tile-by-tile frame (examples/xor/main.rs:235-254) presents every tile it renders.
     *   VK_RENDER_PRESENT       also write the presented pixel (the target is sized to the backbuffer, as by vk_present(w, h))
     *   VK_RENDER_PRESENT_BGRA  ... and the Bgra8Unorm surface copy (vk_present's also_bgra); implies VK_RENDER_PRESENT
     *   VK_RENDER_PRESENT_ONLY  ... and do NOT store the HDR pixel: the backbuffer keeps what it held; implies VK_RENDER_PRESENT
     * Equal to vk_render followed by vk_present(width, height) on every pixel that pass samples at a texel centre; its f32 pixel
     * coordinates put a few per cent of the samples (52 columns and 43 rows of 1920 x 1080) ~1e-7 of a texel off centre, and there the
     * two may differ by one 8-bit step (a hardware sampler's fixed-point weights read the centre there too). */
    VK_RENDER_PRESENT = 256,
    VK_RENDER_PRESENT_BGRA = 512,
    VK_RENDER_PRESENT_ONLY = 1024,
    /* ABI 5 -- VK_MODE_PROCEDURAL only, a TOLERANCE MODE: hash()'s sine (shaders/xor.wgsl:18-20, `fract(sin(h) * 43758.5453123)`) is the
     * hardware's v_sin_f32 behind a multiply by 1 / 2 pi and a fract -- what a GPU running the shader as written computes -- instead of the
     * specified one (f64 Cody-Waite, shared bit for bit with the oracle).  At the hash's arguments (up to ~8e5) that sine keeps a few correct
     * bits and the hash multiplies the rest by 43758: the frame shows a different noise field with the same statistics (C3 at 1080p: mean
     * colour within 0.3 %, 8 x 8-blurred correlation 0.986, mean |d| 0.017, max 0.17), 2.3x faster (1.51 -> 0.65 ms).  Not comparable pixel
     * by pixel with anything; ignored by the other modes; refused with COUNT. */
    VK_RENDER_DEVICE_SINE = 2048
};

/* ---- context: replaces Context::new device/queue setup, src/context.rs:71-181 ---------- */
int vk_ctx_create(int device_ordinal, vk_ctx **out);
int vk_ctx_destroy(vk_ctx *ctx);
/* Run on a caller-owned HIP stream (e.g. torch's current stream); NULL = the context's own.
 * Stream discipline: every call is asynchronous on the context's stream unless it returns host data.  The context's own
 * stream is non-blocking -- it does NOT synchronise with the legacy default stream -- so device buffers the caller fills
 * (or reads) on another stream need an event / synchronisation of the caller's making, or a shared stream set here. */
int vk_ctx_set_stream(vk_ctx *ctx, void *hip_stream);
int vk_ctx_sync(vk_ctx *ctx);
/* Context::get_info, src/context.rs:183-203 */
int vk_device_info(vk_ctx *ctx, char *name, size_t name_cap, int *compute_units, int *arch_is_gfx950,
                   size_t *total_mem_bytes);
/* Message for the last failing call on this context (ctx == NULL: last vk_ctx_create failure). */
const char *vk_last_error(vk_ctx *ctx);
int vk_abi_version(void);

/* ---- inputs ------------------------------------------------------------------------------ */
/* VolumeTexture::new: create_texture + queue.write_texture, src/context/volume_texture.rs:32-59.
 * `host` is the dense x-fastest array (index x + nx*(y + ny*z)); `host2` only for RGBA16F_PAIR
 * (normals).  The library re-lays it out on the device (layout) and builds the skip maps.
 * RGBA16F_PAIR accepts VK_LAYOUT_LINEAR (two dense arrays) or VK_LAYOUT_PACKED (16-byte density+normals
 * records in 4^3 bricks, <= 1.25 GiB; the AUTO choice up to that size). */
int vk_volume_upload(vk_ctx *ctx, const void *host, const void *host2, uint32_t nx, uint32_t ny, uint32_t nz,
                     int format, int layout);
/* Same, but the dense source already lives in device memory of this GPU (large synthetic volumes). */
int vk_volume_upload_device(vk_ctx *ctx, const void *dev, const void *dev2, uint32_t nx, uint32_t ny,
                            uint32_t nz, int format, int layout);
/* Deterministic synthetic volume generated on the device, integer arithmetic only (bit-identical
 * to the oracle's vo_volume_* and to vokselis_amd/volumes.py).  The reference embeds its volume
 * with include_bytes! (volume_texture.rs:33) and that file is absent from the checkout, so the
 * bench and the tests use these.  FOG: u8 in [lo, lo+span) / f16 bit patterns 0x2D1F + h % 656.
 * BONSAI_STANDIN: pot / trunk / canopy / speckled air, u8.
 * FOG_DENSE_CORE: the fog with a dense ball at the centre (radius: a quarter of the smallest dimension; u8 232 + h % 24,
 * f16 0x3B9A + h % 64), the "dense-core variant" of C4 / C5: rays that reach it leave the loop by the
 * reference's opacity early-out (raycast_naive.wgsl:115-117). */
enum vk_generator { VK_GEN_FOG = 0, VK_GEN_BONSAI_STANDIN = 1, VK_GEN_FOG_DENSE_CORE = 2 };
int vk_volume_generate(vk_ctx *ctx, int kind, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t seed,
                       uint32_t lo, uint32_t span, int layout);
/* XorCompute (examples/xor/xor_compute.rs:93-200): one dispatch of shaders/xor.wgsl `cs_main` at
 * un.time = time (0 in the reference: the pass runs before the first Context::update),
 * filling the two rgba16float storage textures (density, normals) the compute raycast reads. */
int vk_volume_generate_xor(vk_ctx *ctx, uint32_t nx, uint32_t ny, uint32_t nz, float time);
/* Share of the cells that are exactly transparent under the transfer function (packed layouts).  Built-in transfer: a cell
 * is empty iff each of its 8 taps is (R8: <= 25; R16_UNORM: <= 6553; R16F: finite and <= 0.1 -- a NaN or infinite tap is never empty). */
int vk_volume_empty_fraction(vk_ctx *ctx, double *fraction);
int vk_volume_info(vk_ctx *ctx, uint32_t dims[3], int *format, int *layout, size_t *device_bytes);

/* Runtime transfer function of VK_MODE_NAIVE_TRILINEAR: a context-wide RGBA table that replaces the built-in transfer and
 * palette (min(0.9, v), smoothstep, the cosine "vertigo" palette: raycast_naive.wgsl:104-110) until it is reset.
 * rgba: n entries of 4 floats (r, g, b, a), not premultiplied, alpha in [0, 1], spread evenly over the sample values
 * [lo, hi] (R8 and R16_UNORM volumes: the normalised value, as the shader sees it; R16F: the value).  Per step, with x the filtered sample
 * on the kernel's scale (R8: 0..255, S = 255; R16_UNORM: 0..65535, S = 65535; R16F: the value, S = 1) and k1 = (n-1) / ((hi-lo) S), k2 = -lo (n-1) / (hi-lo)
 * rounded once to f32:  u = min(max(fma(x, k1, k2), 0), n-1);  i = min(floor(u), n-2);  c = lerp(T[i], T[i+1], u - i);
 * w = (1 - A) c.a;  C += w c.rgb;  A += w  -- the early-out, the sRGB step and the miss colour as without a table.
 * The skip maps and vk_volume_empty_fraction follow the table: a cell is empty iff its taps are finite and every entry
 * from floor(u(min tap)) - 1 to floor(u(max tap)) + 2 has alpha 0.
 * rgba == NULL resets to the built-in transfer.  VK_ERR_INVALID (the previous table stays in force): 2 <= n <=
 * VK_TF_MAX_ENTRIES violated, a non-finite entry, a colour beyond +-VK_TF_MAX_COLOUR, an alpha outside [0, 1], !(lo < hi) or non-finite bounds, or a call
 * between vk_frame_begin and vk_frame_end.  Otherwise the call drains every frame slot (as vk_ctx_sync), stores the table
 * and rebuilds the skip maps of the current volume; frames recorded before it render with the old table.  The table stays
 * in force across vk_volume_upload / _upload_device / vk_volume_generate.  Layouts: LINEAR, PACKED, PACKED_PAIRS; NAIVE
 * renders of BRICKED / QUADS / STAGED volumes, and VK_RENDER_FAST_WALK, are VK_ERR_UNSUPPORTED while a table is set.
 * COMPUTE_NEAREST and PROCEDURAL ignore it. */
#define VK_TF_MAX_ENTRIES 256
#define VK_TF_MAX_COLOUR 1e30f /* |r|, |g|, |b| at most this: the difference of two neighbouring entries stays finite */
int vk_set_transfer_function(vk_ctx *ctx, const float *rgba, uint32_t n, float lo, float hi);

/* Gradient lighting of the table march: shades each sample's table colour by the analytic gradient of the trilinear
 * interpolant (two-sided Blinn-Phong).  It changes only the colour, never the alpha: trip counts,
 * the early-out, skipping and vk_volume_empty_fraction are those of the unlit table.  Per sampled step, from the cell's
 * taps t0..t7 (bit 0 = x, bit 1 = y, bit 2 = z), weights fx, fy, fz, x-lerps c00, c10, c01, c11 and y-lerps l0, l1,
 * each operation rounded once:  e0 = fma(fy, (t3-t2) - (t1-t0), t1-t0);  e1 = fma(fy, (t7-t6) - (t5-t4), t5-t4);
 * g = (fma(fz, e1 - e0, e0) nx, fma(fz, y1 - y0, y0) ny, (l1 - l0) nz) with y0 = c10 - c00, y1 = c11 - c01;
 * q = g.g.  If q is finite and >= FLT_MIN: N = g rsqrt(q), diff = |N.L|, spec = |N.H|^shininess; otherwise (no
 * gradient) diff = 1, spec = 0.  rgb' = c.rgb (ambient + diffuse diff) + specular spec, composited as c.rgb is.
 * L = dir normalised (in double, rounded once per component), or -ray for a headlight; V = -ray; H = normalise(L + V)
 * once per ray (V if L + V is zero).
 * light == NULL turns lighting off.  VK_ERR_INVALID (the previous lighting stays in force): a field not finite, a
 * zero-length dir with headlight == 0, ambient / diffuse / specular outside [0, 16], shininess outside [1, 1024].
 * headlight != 0 puts the light at the eye (dir is then ignored).  Lighting is host state, taken into the kernel
 * arguments when a render is recorded: the call needs no drain and no map rebuild, and it may be made at any time,
 * between vk_frame_begin and vk_frame_end too (renders recorded before it keep the old lighting, renders after it
 * take the new).  While lighting is set, NAIVE_TRILINEAR renders need a transfer function (VK_ERR_UNSUPPORTED
 * otherwise); COMPUTE_NEAREST and PROCEDURAL ignore it. */
typedef struct vk_lighting {
    float dir[3];       /* towards the light, world space (the unit cube); ignored with headlight */
    int32_t headlight;  /* != 0: the light sits at the eye, L = -ray direction */
    float ambient, diffuse, specular, shininess;
} vk_lighting; /* 32 bytes */
int vk_set_lighting(vk_ctx *ctx, const vk_lighting *light);

/* Projection of VK_MODE_NAIVE_TRILINEAR: VK_PROJ_COMPOSITE (default), the front-to-back compositing of the reference, or
 * VK_PROJ_MAX, a maximum-intensity projection over the window [lo, hi] of the table in force.  Under
 * VK_PROJ_MAX a ray that hits the box carries U = +0 and takes, per iteration of the reference's loop, with x the filtered
 * sample and k1, k2 as under vk_set_transfer_function:  U = max(U, min(max(fma(x, k1, k2), 0), n-1))  (a NaN sample counts as 0;
 * U is +0 whenever it compares equal to zero);  the ray ends after the iteration in which U reaches n-1.  The pixel is
 * i = min(floor(U), n-2);  c = lerp(T[i], T[i+1], U - i);  (srgb(c.r), srgb(c.g), srgb(c.b), 1): the table is read once per
 * ray and its alpha column not at all.  Without a table the implicit grey ramp {(0,0,0), (1,1,1)} over [0, 1] is used (n = 2),
 * bit for bit the frame of that table set explicitly.  Misses are (0,0,0,1).  Lighting (vk_set_lighting) is ignored under
 * VK_PROJ_MAX, with or without a table.  The skip maps and vk_volume_empty_fraction follow the projection: a cell is empty iff
 * its 8 taps are finite and its largest tap M has min(max(fma(M, k1, k2), 0), n-1) == 0.
 * The call drains every frame slot (as vk_ctx_sync), stores the value and rebuilds the skip maps of the current volume under
 * the (projection, table) pair now in force; the order of vk_set_projection and vk_set_transfer_function does not matter.
 * VK_ERR_INVALID (the previous projection stays in force): an unknown value, or a call between vk_frame_begin and
 * vk_frame_end.  The projection stays in force across vk_volume_upload / _upload_device / vk_volume_generate.  Layouts under
 * VK_PROJ_MAX: LINEAR, PACKED, PACKED_PAIRS; NAIVE renders of BRICKED / QUADS / STAGED volumes, and VK_RENDER_FAST_WALK, are
 * VK_ERR_UNSUPPORTED.  COMPUTE_NEAREST and PROCEDURAL ignore it. */
enum vk_projection { VK_PROJ_COMPOSITE = 0, VK_PROJ_MAX = 1 };
int vk_set_projection(vk_ctx *ctx, int projection);
int vk_get_projection(vk_ctx *ctx, int *projection);

/* First-hit isosurface rendering of VK_MODE_NAIVE_TRILINEAR: an opaque surface where the filtered volume
 * first reaches a threshold, the crossing refined by bisection, shaded from the gradient.  While an isosurface is set,
 * NAIVE_TRILINEAR renders are isosurface renders: the transfer table and the projection are ignored (they stay stored --
 * vk_get_projection still reports the stored projection -- and are in force again after vk_set_isosurface(ctx, NULL)); lighting
 * (vk_set_lighting) is honoured, with or without a table.  COMPUTE_NEAREST and PROCEDURAL ignore it.
 * iso_k is the threshold on the kernel's scale, rounded once to f32: R8: iso * 255.0f; R16_UNORM: iso * 65535.0f; R16F: iso.  For a pixel whose ray hits the
 * box, ray, box, t0 = max(t0, 0), dt, p = eye + t0 dir and s = dir * dt are as without an isosurface, and
 *     hit = false; j = 0
 *     for (t = t0; t < t1; t = t + dt) {           the reference's loop
 *         x = trilinear(V, p)                      the filter of every other render, bit for bit
 *         if (x >= iso_k) { hit = true; break; }   a NaN sample is no hit; the break comes before p is advanced
 *         p = p + s;  j = j + 1
 *     }
 *     if (!hit) out = (0, 0, 0, 1)                 as a miss
 *     else {
 *         a = 0                                    how far back towards the eye the surface lies, in steps: a dyadic in [0, 1)
 *         if (j >= 1)                              a hit in the ray's first iteration is not refined (the cut face of the box)
 *             for (i = 1; i <= refine; i++) {
 *                 m = a + 2^-i
 *                 q = (fma(-m, s.x, p.x), fma(-m, s.y, p.y), fma(-m, s.z, p.z))
 *                 if (trilinear(V, q) >= iso_k) a = m
 *             }
 *         q = fma(-a, s, p) per component
 *         g = the gradient of the sample at q, as under vk_set_lighting
 *         c = rgb;  with lighting set: c = c (ambient + diffuse diff) + specular spec   (two-sided; no gradient: diff = 1, spec = 0)
 *         out = (srgb(c.r), srgb(c.g), srgb(c.b), 1)
 *     }
 * The texel indices of a refinement sample are clamped to the edge like any sample's.  The per-pixel step count (VK_RENDER_COUNT) is
 * the number of loop iterations executed, the hitting one included; S_sampled counts the iterations that fetched taps; the
 * refinement and shading samples count in neither.  The skip maps and vk_volume_empty_fraction follow the isosurface: a cell is
 * empty iff its 8 taps are finite and its largest tap lies below iso_k.
 * The call drains every frame slot (as vk_ctx_sync), stores the value and rebuilds the skip maps of the current volume under the
 * predicate now in force: the isosurface's when one is set, otherwise that of the (projection, table) pair.  The order of
 * vk_set_isosurface, vk_set_projection and vk_set_transfer_function does not matter.  iso == NULL turns the isosurface off.
 * VK_ERR_INVALID (the previous state stays in force): a non-finite iso, a colour that is not finite or beyond +-VK_TF_MAX_COLOUR,
 * refine > VK_ISO_MAX_REFINE, or a call between vk_frame_begin and vk_frame_end.  The state stays in force across vk_volume_upload /
 * _upload_device / vk_volume_generate.  Layouts: LINEAR, PACKED, PACKED_PAIRS; NAIVE renders of BRICKED / QUADS / STAGED volumes,
 * and VK_RENDER_FAST_WALK, are VK_ERR_UNSUPPORTED while an isosurface is set.
 * vk_get_isosurface: *enabled (may be NULL) says whether one is set; *out (may be NULL) receives it when one is. */
#define VK_ISO_MAX_REFINE 16
typedef struct vk_isosurface {
    float iso;       /* threshold in sample values, the units of vk_set_transfer_function's lo / hi (R8, R16_UNORM: the normalised value; R16F: the value) */
    float rgb[3];    /* linear surface colour, not premultiplied; finite, |c| <= VK_TF_MAX_COLOUR */
    uint32_t refine; /* bisection steps R at the hit, 0 .. VK_ISO_MAX_REFINE */
} vk_isosurface;     /* 20 bytes */
int vk_set_isosurface(vk_ctx *ctx, const vk_isosurface *iso);
int vk_get_isosurface(vk_ctx *ctx, vk_isosurface *out, int *enabled);

/* Light-direction shadows of the first-hit isosurface: a ray that hit casts one more isosurface ray from its
 * refined crossing towards the light, and a point whose shadow ray hits keeps 1 - strength of its diffuse and specular terms.
 * They take effect on a NAIVE_TRILINEAR render only when an isosurface is set, lighting is set and the light is not a headlight (a
 * headlight's shadow ray runs back along the primary ray, which was empty up to the hit).  In every other case -- unlit isosurface,
 * headlight, table / lit / MAX / built-in renders, COMPUTE_NEAREST, PROCEDURAL -- the state is stored and ignored, and the render
 * launches the kernels it launches without shadows, bit for bit.
 * For a ray that hit, with q the refined crossing (a first-iteration hit: p itself), g the gradient, L = (lx, ly, lz) the unit light
 * direction, iso_k the threshold and [lo, hi] the box the primary ray marched (the clip box when one is set, else the unit cube), every
 * operation one f32 rounding:
 *     dts = dt_scale * min(1 / (nx |L.x|), 1 / (ny |L.y|), 1 / (nz |L.z|))       the primary ray's dt formula with L for dir
 *     intersect_box(q, L, lo, hi) -> tb0, tb1                                    the same function, the same operations
 *     shadowed = false
 *     if (!(tb0 > tb1)) {
 *         ts0 = max(max(tb0, 0), bias * dts)
 *         ps = (fma(ts0, L.x, q.x), fma(ts0, L.y, q.y), fma(ts0, L.z, q.z));  ss = L * dts
 *         for (t = ts0; t < tb1; t = t + dts) {
 *             if (trilinear(V, ps) >= iso_k) { shadowed = true; break; }         the filter of every other render; NaN is no hit
 *             ps = ps + ss
 *         }
 *     }
 *     k = shadowed ? 1 - strength : 1
 *     rgb' = c.rgb * (ambient + (diffuse * diff) * k) + (specular * spec) * k    diff, spec as under vk_set_lighting; no gradient: diff = 1, spec = 0
 * A point facing away from the light marches into its own material and is shadowed: with the two-sided |N.L| this is what keeps the
 * far side of an object from lighting up.  bias = 0 samples q itself, which is at or above the threshold by the bisection's invariant:
 * every hit pixel is then shadowed.  Shadow iterations count in neither the per-pixel step image nor S_ref / S_sampled.  The skip maps
 * are the isosurface's and stay exact for the shadow ray (the same filter, the same compare, one map per octant).
 * The state rules are lighting's: pure host state read when a render is recorded -- no drain, no map rebuild, settable at any time,
 * between vk_frame_begin and vk_frame_end too (renders recorded before the call keep the old value) -- and it stays in force across
 * vk_volume_upload / _upload_device / vk_volume_generate.  s == NULL turns shadows off.  VK_ERR_INVALID (the previous state stays in
 * force): a non-finite field, strength outside [0, 1], bias outside [0, VK_SHADOW_MAX_BIAS].  Layouts and flags are the isosurface's.
 * vk_render, vk_render_partition, vk_render_batch, frames in flight, the fused present and vk_group_render honour it; the ranks of a
 * partition and the members of a group need the same value on every context (as for the clip box).
 * vk_get_shadows: *enabled (may be NULL) says whether shadows are set; *out (may be NULL) receives them when they are. */
#define VK_SHADOW_MAX_BIAS 1024
typedef struct vk_shadows {
    float strength; /* 0 .. 1: how much of the diffuse and specular terms a shadowed point loses */
    float bias;     /* 0 .. VK_SHADOW_MAX_BIAS: distance of the first shadow sample from the surface, in shadow steps */
} vk_shadows;       /* 8 bytes */
int vk_set_shadows(vk_ctx *ctx, const vk_shadows *s);
int vk_get_shadows(vk_ctx *ctx, vk_shadows *out, int *enabled);

/* A clip box (cut-away, region of interest) of the table, lit, MAX and isosurface marches: NAIVE_TRILINEAR rays of those renders march
 * the box [lo, hi], given in unit-cube coordinates, instead of the unit cube.  intersect_box takes box_min = lo and box_max = hi per
 * axis, in the same f32 operations:
 *     inv = 1 / d[i];  a = (lo[i] - o[i]) * inv;  b = (hi[i] - o[i]) * inv;  tmin[i] = fmin(a, b);  tmax[i] = fmax(a, b)
 *     t0 = max(tmin[0], tmin[1], tmin[2]);  t1 = min(tmax[0], tmax[1], tmax[2])
 * and everything after it is as without a box: t0 > t1 is a miss, (0, 0, 0, 1); t0 = max(t0, 0); dt comes from the direction and the
 * volume's dimensions alone; the loop runs for (t = t0; t < t1; t = t + dt) from p = eye + t0 dir; the family's loop and epilogue are
 * unchanged.  Under an isosurface, "a hit in the ray's first iteration is not refined" now also means the cut face of the clip box.
 * The box lo = (0, 0, 0), hi = (1, 1, 1) gives bit for bit the frame and the step counts of no box.
 * box == NULL turns the box off.  VK_ERR_INVALID (the previous box stays in force): a component that is not finite, or
 * 0 <= lo[i] < hi[i] <= 1 fails on an axis.
 * The box is host state like lighting, taken into the kernel arguments -- and into the host's screen-space geometry: cull rectangle,
 * active tiles and tile order follow the box's projected corners -- when a render is recorded: no drain, no map rebuild, it may be set
 * at any time, between vk_frame_begin and vk_frame_end too (renders recorded before the call keep the old box), and it stays in force
 * across vk_volume_upload / _upload_device / vk_volume_generate.  The skip maps and vk_volume_empty_fraction do not depend on it.
 * NAIVE renders of the table, lit, MAX and isosurface kernels honour it (LINEAR, PACKED, PACKED_PAIRS).  A NAIVE render that would
 * launch the built-in march -- no table, the compositing projection, no isosurface, on any layout -- is VK_ERR_UNSUPPORTED while a box
 * is set.  COMPUTE_NEAREST and PROCEDURAL ignore it.  vk_partition_active, vk_partition_order, vk_render_partition, vk_render_batch,
 * vk_untile* and vk_group_render follow the context's box: the ranks of a partition, and the members of a group, need the same box on
 * every context (as for vk_partition_wire).  vk_tiles_active keeps the unit cube; vk_tiles_active_clip is vk_tiles_active under a box
 * (NULL: the unit cube; VK_ERR_INVALID for a box vk_set_clip_box would refuse).
 * vk_get_clip_box: *enabled (may be NULL) says whether one is set; *out (may be NULL) receives it when one is. */
typedef struct vk_clip_box {
    float lo[3], hi[3]; /* unit-cube coordinates, 0 <= lo[i] < hi[i] <= 1 */
} vk_clip_box;          /* 24 bytes */
int vk_set_clip_box(vk_ctx *ctx, const vk_clip_box *box);
int vk_get_clip_box(vk_ctx *ctx, vk_clip_box *out, int *enabled);
int vk_tiles_active_clip(const void *camera144, int mode, uint32_t width, uint32_t height, uint32_t tile_size,
                         const vk_clip_box *box, unsigned char *active, uint32_t *n_active);

/* The geometry pass of the first-hit isosurface: where the surface is.  It needs an isosurface set
 * (vk_set_isosurface) and has VK_MODE_NAIVE_TRILINEAR's semantics.  For a pixel of the tile, the ray, intersect_box (the clip box when one
 * is set), t0 = max(t0, 0), dt, p, s, the loop with its trip budget, the rule that a first-iteration hit is not refined and the
 * bisection a (R = the stored refine) are exactly those of the isosurface colour render above.  The bisection runs ALWAYS, whether or not
 * lighting is set; lighting, shadows, the surface colour, the table and the projection have no influence on the pass.
 * Per pixel the pass writes a 32-byte record of two float4.  For a ray that hit, every operation one f32 rounding:
 *     q = (fma(-a, s.x, p.x), fma(-a, s.y, p.y), fma(-a, s.z, p.z))                  a = 0: p itself
 *     t = fma(q.z - eye.z, dir.z, fma(q.y - eye.y, dir.y, (q.x - eye.x) * dir.x))     the distance of q along the unit ray
 *     g = the gradient of the sample at q, as under vk_set_lighting, in its operation order, on the kernel's scale (R8: taps 0..255,
 *         R16_UNORM: 0..65535, R16F: values), times the volume's dimensions per axis -- NOT normalised
 *     x = trilinear(V, q)                                                             the filtered sample, on the kernel's scale
 *     record = { (q.x, q.y, q.z, t), (g.x, g.y, g.z, x) }
 * A pixel whose ray misses the box or never hits, a pixel of a culled 8x8 block and a pixel of an inactive tile write the miss record
 * { (0, 0, 0, +inf), (0, 0, 0, 0) }: isfinite(t) is the hit mask.  Pixels outside the tile are not written.
 * The normal is left to the consumer: the outward normal of a surface entered from below the threshold is -g / |g|.  On the cut face of
 * the box or the clip box (a first-iteration hit) g is still the data's gradient, not the face's normal.  The gradient is stored raw:
 * its length serves edge detection and a "no gradient" test (g = 0).  The skip maps are the isosurface's and stay exact (the same operator
 * and predicate); the pass triggers no map rebuild.
 * The geometry surface, [height][width] records, belongs to the frame slot like the step image: it is allocated, and filled with the miss
 * record, by the slot's first geometry pass at the backbuffer's size, and freed by vk_backbuffer_resize, vk_ctx_frames_in_flight and
 * vk_ctx_destroy.  Between vk_frame_begin and vk_frame_end the pass goes to that frame's slot and stream.
 * vk_render_geometry is asynchronous on the slot's stream and touches neither the backbuffer, the present targets, the step image nor
 * the counters.  flags: VK_RENDER_NO_SKIP, VK_RENDER_SAFE, VK_RENDER_FORCE_SKIP, VK_RENDER_PROBE_ALWAYS -- the default skip policy is the
 * colour render's, from the census -- and the records are identical under every combination of them.  VK_RENDER_FAST_WALK and a BRICKED /
 * QUADS / STAGED volume are VK_ERR_UNSUPPORTED; any other flag, no isosurface set, no volume, no backbuffer, no camera: VK_ERR_INVALID.
 * vk_geometry_info (does not synchronise) and vk_readback_geometry (blocking; row_pitch_bytes >= width * 32) are VK_ERR_INVALID before
 * the slot's first geometry pass since the last resize; vk_frame_geometry reads a frame's surface under vk_frame_readback's rules.
 * vk_pick (blocking) renders the 1 x 1 tile at (x, y) into the current slot's surface and downloads that record: bit for bit the
 * full-frame pass's record of the pixel (the ray does not depend on the tile).  x >= width or y >= height: VK_ERR_INVALID.
 * vk_render_partition, vk_render_batch, vk_group_render and the fused present have no geometry output. */
typedef struct vk_hit {
    int32_t hit;   /* 1: isfinite(t) */
    float pos[3];  /* q, unit-cube coordinates */
    float t;       /* distance along the unit ray; +inf for a miss */
    float grad[3]; /* g, raw */
    float value;   /* x */
} vk_hit;          /* 36 bytes */
int vk_render_geometry(vk_ctx *ctx, int32_t tile_x, int32_t tile_y, uint32_t tile_w, uint32_t tile_h, float dt_scale, uint32_t flags);
int vk_geometry_info(vk_ctx *ctx, uint32_t *width, uint32_t *height, void **device_ptr);
int vk_readback_geometry(vk_ctx *ctx, void *dst, size_t row_pitch_bytes);
int vk_frame_geometry(vk_ctx *ctx, uint64_t frame_id, void *dst, size_t row_pitch_bytes);
int vk_pick(vk_ctx *ctx, uint32_t x, uint32_t y, float dt_scale, vk_hit *out);

/* The slice pass: a plane through the volume -- axial, coronal, sagittal or oblique -- windowed by the table in
 * force, optionally a thick slab reduced by maximum, minimum or mean.  No ray: the pass needs no camera, and lighting, isosurface, shadows,
 * projection and uniform have no influence.  Only the clip box is honoured.  The plane arrives per call, so three orthogonal views and a
 * 3-D render can share one backbuffer, a tile each.
 * For backbuffer pixel (px, py) of the tile, in absolute backbuffer coordinates (a pixel's result never depends on the tile), every
 * operation one f32 rounding, fma fused:
 *     P.c = fma((float)py, dv.c, fma((float)px, du.c, origin.c))                        c = x, y, z
 *     inside = lo.c <= P.c && P.c <= hi.c on all three axes          [lo, hi]: the clip box when one is set, else [0, 1]^3; a NaN is outside
 *     outside: out = (0, 0, 0, 1), value record (+0, 0)               the clear colour, like a miss
 *     samples == 1:  x = trilinear(V, P)
 *     otherwise, for k = 0 .. samples - 1:
 *         w = (float)k - 0.5f * (float)(samples - 1);  Pk.c = fma(w, dn.c, P.c);  xk = trilinear(V, Pk)
 *                                                      texel indices clamp to the edge like any sample's; no inside test per sample
 *         VK_SLAB_MAX:  M starts at -inf;  M = (xk > M) ? xk : M;  x = M                a NaN sample is passed over; all NaN leaves -inf
 *         VK_SLAB_MIN:  M starts at +inf;  M = (xk < M) ? xk : M;  x = M
 *         VK_SLAB_MEAN: acc starts at +0;  acc = acc + xk in the order of k;  x = acc * rn,  rn = (float)(1.0 / (double)samples)
 *     U = fmin(u > 0 ? u : +0, umax),  u = fma(x, k1, k2)             the running maximum of VK_PROJ_MAX after one sample: a NaN and
 *                                                                     anything <= 0 read entry 0
 *     i = min(floor(U), n - 2);  f = U - i;  c = fma(f, T[i+1] - T[i], T[i]) per channel;  no table: the grey ramp, c = U
 *     out = (linear_to_srgb(c.r), linear_to_srgb(c.g), linear_to_srgb(c.b), 1);  value record (x, 1)
 * trilinear is the filter of every other render, bit for bit, and x is on the kernel's scale (R8: 0..255, R16_UNORM: 0..65535, R16F: the
 * value); k1, k2, umax are those of the table in force (vk_set_transfer_function) for the volume's format.
 * vk_render_slice is asynchronous on the current slot's stream (between vk_frame_begin and vk_frame_end: that frame's), writes only the
 * tile's pixels of the backbuffer -- tile pixels outside the backbuffer are dropped -- and touches no step image, counters, present
 * targets or geometry surface.  flags: VK_SLICE_VALUES, under which it also writes the pixels' value records into the VALUE SURFACE,
 * [height][width] records of two f32 (x, weight): what a viewer reads the number under the cursor from.  The value surface belongs to the
 * frame slot like the geometry surface: allocated and zero-filled by the slot's first such pass, freed by vk_backbuffer_resize,
 * vk_ctx_frames_in_flight and vk_ctx_destroy.
 * VK_ERR_INVALID (the backbuffer is untouched): a NULL slice, a component that is not finite or beyond +-VK_SLICE_MAX_COORD (dn: when
 * samples > 1), samples outside 1 .. VK_SLICE_MAX_SAMPLES, an unknown reduce with samples > 1, any flag other than VK_SLICE_VALUES, no
 * volume, no backbuffer.  VK_ERR_UNSUPPORTED: a BRICKED / QUADS / STAGED or RGBA16F_PAIR volume (the pass has kernels for LINEAR, PACKED
 * and PACKED_PAIRS).
 * vk_slice_values_info (does not synchronise) and vk_readback_slice_values (blocking; row_pitch_bytes >= width * 8) are VK_ERR_INVALID
 * before the slot's first pass with VK_SLICE_VALUES since the last resize; vk_frame_slice_values reads a frame's surface under
 * vk_frame_readback's rules.  vk_slice_probe (blocking) renders the 1 x 1 tile at (x, y) with VK_SLICE_VALUES and downloads its record:
 * bit for bit the full-frame pass's; x >= width or y >= height: VK_ERR_INVALID.
 * vk_render_partition, vk_render_batch, vk_group_render and the fused present have no slice output. */
#define VK_SLICE_MAX_SAMPLES 256
#define VK_SLICE_MAX_COORD 1e6f
enum { VK_SLAB_MAX = 0, VK_SLAB_MIN = 1, VK_SLAB_MEAN = 2 };
enum { VK_SLICE_VALUES = 1 };
typedef struct vk_slice {
    float origin[3];   /* the position of the CENTRE of backbuffer pixel (0, 0), unit-cube coordinates */
    float du[3];       /* position change per pixel in +x */
    float dv[3];       /* position change per pixel in +y */
    float dn[3];       /* position change per slab sample (ignored when samples == 1) */
    uint32_t samples;  /* 1 .. VK_SLICE_MAX_SAMPLES */
    int32_t reduce;    /* VK_SLAB_MAX / _MIN / _MEAN (ignored when samples == 1) */
} vk_slice;            /* 56 bytes */
typedef struct vk_slice_sample {
    int32_t inside; /* 1: P lies in the box */
    float pos[3];   /* P */
    float value;    /* x; +0 outside */
} vk_slice_sample;  /* 20 bytes */
int vk_render_slice(vk_ctx *ctx, const vk_slice *slice, int32_t tile_x, int32_t tile_y, uint32_t tile_w, uint32_t tile_h, uint32_t flags);
int vk_slice_values_info(vk_ctx *ctx, uint32_t *width, uint32_t *height, void **device_ptr);
int vk_readback_slice_values(vk_ctx *ctx, void *dst, size_t row_pitch_bytes);
int vk_frame_slice_values(vk_ctx *ctx, uint64_t frame_id, void *dst, size_t row_pitch_bytes);
int vk_slice_probe(vk_ctx *ctx, const vk_slice *slice, uint32_t x, uint32_t y, vk_slice_sample *out);

/* The histogram and region statistics of the volume: where the data lies -- what a caller needs to choose the
 * domain of vk_set_transfer_function, an isovalue or a slice's window, and the mean and deviation of a region.  A reduction over the
 * STORED texels (no filter, no ray, no plane) of the voxel box [x0, x1) x [y0, y1) x [z0, z1); the box must lie within the volume and
 * may be empty; a NULL box is the whole volume.  Each voxel is counted once, whatever the layout duplicates.  For a voxel's texel t as
 * f32 on the kernel's scale (R8: 0..255, R16_UNORM: 0..65535, R16F: the value -- the scale of vk_slice_sample.value):
 *     S    = 255 / 65535 / 1
 *     lo_k = (float)((double)lo * S),  hi_k = (float)((double)hi * S)
 *     k1   = (float)(bins / (((double)hi - (double)lo) * S)),  k2 = (float)(-(double)lo * bins / ((double)hi - (double)lo))
 *                                                     formed on the host in double, rounded once
 *     t is a NaN   -> n_nan
 *     t <  lo_k    -> n_below
 *     t >  hi_k    -> n_above                         (+-inf land here; the top is closed, like numpy.histogram's)
 *     otherwise    -> counts[min((int)floorf(fmaf(t, k1, k2)), bins - 1)], never below 0     (-0 at lo_k = 0 is bin 0)
 *     min, max     over every texel that is not a NaN, in the order in which -0 lies below +0 (an empty box or all NaN: min = +inf,
 *                  max = -inf)
 *     sum, sum_sq  f64 sums of t and t * t (the product in f64) over the FINITE texels; n_finite their number
 * So an R8 volume with bins = 256 over [0, 1] has counts == bincount(v), an R16_UNORM volume counts == bincount(v >> 8).
 * Counts, categories, min and max are integers or selections: the same on every layout and every run, bit for bit.  The sums are exact
 * for the integer formats while they stay below 2^53; for R16F they are f64 sums in an order that depends on the launch, the same from
 * run to run on one device (no float atomics).
 * vk_volume_histogram is blocking; it runs on the context's current stream behind whatever was recorded there and changes no context
 * state: no surface, counter or frame slot is touched.  counts (bins entries) may be NULL: statistics only.  stats may be NULL.
 * flags: VK_HIST_CLIP_BOX -- the voxel box is derived from the clip box in force (box must be NULL): a voxel belongs to it when its
 * centre (i + 0.5) / n lies in the clip box's closed interval on every axis (the index range is formed on the host in double); no clip
 * box set: the whole volume.
 * VK_ERR_INVALID, decided before any launch, outputs untouched: a NULL request, bins outside 1 .. VK_HIST_MAX_BINS, lo or hi not
 * finite or hi <= lo, an unknown flag, a box that is inverted or leaves the volume, a box together with VK_HIST_CLIP_BOX, no volume.
 * VK_ERR_UNSUPPORTED ("histogram: ..."): a BRICKED / QUADS / STAGED or RGBA16F_PAIR volume -- the set the slice pass refuses.
 * vk_histogram_window is host arithmetic and needs no context: the window [w_lo, w_hi] that holds the percentiles p_lo .. p_hi of a
 * histogram over [lo, hi].  N = sum(counts); r_lo = floor(p_lo N), b_lo the first bin whose running total exceeds r_lo; r_hi =
 * ceil(p_hi N), b_hi the first bin whose running total reaches r_hi, not less than b_lo; w_lo = lo + b_lo (hi - lo) / bins, w_hi =
 * lo + (b_hi + 1)(hi - lo) / bins, in double, each rounded once to f32.  VK_ERR_INVALID: a NULL argument, bins outside
 * 1 .. VK_HIST_MAX_BINS, lo or hi not finite or hi <= lo, N == 0, not 0 <= p_lo < p_hi <= 1, a rounded w_lo >= w_hi (its message is
 * read with vk_last_error(NULL)). */
#define VK_HIST_MAX_BINS 4096
enum { VK_HIST_CLIP_BOX = 1 };
typedef struct vk_histogram {
    float lo, hi;    /* the domain in sample values, like vk_set_transfer_function's */
    uint32_t bins;   /* 1 .. VK_HIST_MAX_BINS */
    uint32_t flags;  /* VK_HIST_CLIP_BOX */
} vk_histogram;      /* 16 bytes */
typedef struct vk_voxel_box {
    uint32_t x0, y0, z0, x1, y1, z1;
} vk_voxel_box;      /* 24 bytes */
typedef struct vk_volume_stats {
    uint64_t n_voxels, n_nan, n_below, n_above, n_finite;
    double sum, sum_sq;  /* on the kernel's scale */
    float min, max;      /* on the kernel's scale */
    float scale;         /* S: divide by it (sum_sq by its square) for sample values */
    uint32_t pad;
} vk_volume_stats;       /* 72 bytes */
int vk_volume_histogram(vk_ctx *ctx, const vk_histogram *hist, const vk_voxel_box *box, uint64_t *counts, vk_volume_stats *stats);
int vk_histogram_window(const uint64_t *counts, uint32_t bins, float lo, float hi, double p_lo, double p_hi, float *w_lo, float *w_hi);

/* The isosurface as a triangle mesh, by marching tetrahedra: the surface the first-hit render shows, handed over.
 * Every f32 operation below is rounded once and nothing is fused.
 * Box.  `box` is a voxel box [x0, x1) x [y0, y1) x [z0, z1) under vk_volume_histogram's rules: it lies within the volume, may be empty,
 * NULL is the whole volume, and VK_MESH_CLIP_BOX derives it from the clip box exactly as VK_HIST_CLIP_BOX does.  A cube is a low-corner
 * voxel (x, y, z) with x0 <= x < x1 - 1, likewise on y and z; its 8 corners are the stored texels V(x+i, y+j, z+k) as f32 on the kernel's
 * scale (R8 0..255, R16_UNORM 0..65535, R16F the value).  A box thinner than 2 voxels on an axis has no cubes.  The surface is open where
 * it leaves the box (no caps).
 * Threshold.  iso_k is formed from iso exactly as vk_set_isosurface does: iso * 255.0f, iso * 65535.0f, or iso.  A corner is inside iff
 * v >= iso_k, the render's hit predicate.
 * Empty cubes.  A cube with a corner that is NaN or infinite emits nothing; a cube whose corners are all inside or all outside emits
 * nothing.
 * Tetrahedra.  Otherwise, k = 0..5 in this order; pi_k is the k-th permutation of the axes in lexicographic order: (x,y,z), (x,z,y),
 * (y,x,z), (y,z,x), (z,x,y), (z,y,x).  The tetrahedron has vertices v0 = (0,0,0), v1 = v0 + e[pi_k(0)], v2 = v1 + e[pi_k(1)], v3 =
 * (1,1,1), as offsets from the low corner.  mask has bit i set iff v_i is inside; masks 0 and 15 emit nothing, otherwise the triangles
 * of T[mask] in order, each three tetrahedron edges (a,b) with a < b; for an odd permutation (k = 1, 2, 5) the second and third vertex of
 * every triangle are swapped.
 *     mask  1: (01,02,03)             mask  8: (03,23,13)
 *     mask  2: (01,13,12)             mask  9: (01,02,23) (01,23,13)
 *     mask  3: (02,03,13) (02,13,12)  mask 10: (01,23,12) (01,03,23)
 *     mask  4: (02,12,23)             mask 11: (02,23,12)
 *     mask  5: (01,23,03) (01,12,23)  mask 12: (02,12,13) (02,13,03)
 *     mask  6: (01,13,23) (01,23,02)  mask 13: (01,12,13)
 *     mask  7: (03,13,23)             mask 14: (01,03,02)
 * Vertex.  The vertex on edge (a,b) uses the lattice points A = low corner + v_a and B = low corner + v_b; A <= B holds componentwise
 * whichever cube or tetrahedron the edge is seen from, which makes shared vertices bitwise equal.  With vA, vB their texels:
 *     f     = (iso_k - vA) / (vB - vA)                                              a true divide
 *     pos.c = (((float)A.c + 0.5f) + (B.c > A.c ? f : 0.0f)) / (float)n.c          per axis, a true divide
 * Positions are in unit-cube coordinates with texel centres at (i + 0.5) / n: the convention of the march's filter and of vk_hit.pos.
 * f lies in [0, 1].  A vertex that lands on a lattice point yields zero-area triangles, which are kept.
 * Orientation.  (p1 - p0) x (p2 - p0) points from inside to outside, towards lower values: the -g / |g| of the geometry pass.
 * Order.  Cubes in the volume's index order restricted to the box, x fastest, then y, then z; within a cube k = 0..5; within a
 * tetrahedron the table's order.  The output is one array of n triangles x 3 vertices x 3 f32 (36 bytes per triangle), bit for bit
 * the same on every layout, every launch shape and every run.
 * vk_extract_isosurface is blocking; it runs on the context's current stream (inside vk_frame_begin / _end: that frame's), allocates and
 * frees its own buffers and changes no context state: no surface, counter, slot, skip map or stored isosurface; req->iso is independent of
 * vk_set_isosurface.  *n_triangles always receives the total.  triangles == NULL: only the count pass runs.  Otherwise the first
 * min(n, cap_triangles) triangles are written, in order: a truncated call returns a bitwise prefix of the full one.
 * VK_ERR_INVALID, decided before any launch, outputs untouched: a NULL req or n_triangles, a non-finite iso, an unknown flag, a box that
 * is inverted or leaves the volume, a box together with VK_MESH_CLIP_BOX, no volume.  VK_ERR_UNSUPPORTED ("mesh: ..."): a BRICKED /
 * QUADS / STAGED or RGBA16F_PAIR volume -- the set the histogram refuses.  VK_ERR_OOM: the output buffer cannot be allocated. */
enum { VK_MESH_CLIP_BOX = 1 };
typedef struct vk_mesh_request {
    float iso;       /* the threshold in sample values, like vk_isosurface.iso */
    uint32_t flags;  /* VK_MESH_CLIP_BOX */
} vk_mesh_request;   /* 8 bytes */
int vk_extract_isosurface(vk_ctx *ctx, const vk_mesh_request *req, const vk_voxel_box *box, float *triangles, uint64_t cap_triangles, uint64_t *n_triangles);

/* The volume filter pass: the volume the context holds into another volume of the same dimensions and format -- a
 * separable convolution (a Gaussian smooth, a sharpen) or a 3x3x3 median -- so that the isosurface, the mesh, the histogram and every
 * march see denoised data without a round trip through the host.  Every f32 operation below is rounded once; fmaf is fused where
 * written and nothing else is.
 * t(x, y, z) is the STORED texel as f32 on the kernel's scale (R8 0..255, R16_UNORM 0..65535, R16F the value); indices are clamped to the
 * edge per axis, c(i, n) = min(max(i, 0), n - 1).
 * VK_FILTER_CONVOLVE.  Three axis passes in the order x, y, z over unrounded f32 intermediates, never requantised.  An axis with radius
 * 0 is skipped entirely and its weights are not read.  For the x axis, r = radius[0], w = weights[0]:
 *     acc = w[0] * t(c(x - r, nx), y, z)
 *     for k = 1 .. 2 r:  acc = fmaf(w[k], t(c(x - r + k, nx), y, z), acc)
 *     a(x, y, z) = acc
 * the y pass runs the same loop over a with clamped y, the z pass over that result with clamped z.  (Clamping the index of an
 * intermediate is taking the intermediate of the clamped voxel: the rule does not say whether one kernel or three run.)
 * Store, v the final value:  R8 (uint8) rintf(fminf(fmaxf(v, 0.0f), 255.0f)), ties to even; R16_UNORM the same with 65535 (with the
 * weight bound and radius <= VK_FILTER_MAX_RADIUS v is finite for the integer formats); R16F f32 -> f16 round to nearest even, f16
 * denormals kept, overflow +-inf, any NaN stored as 0x7E00.  f32 denormals are kept (the library is built without flush-to-zero).  With
 * all three radii 0 the output is the stored volume bit for bit, NaN payloads apart.
 * VK_FILTER_MEDIAN3.  The output texel is the 14th smallest of the 27 stored texels t(c(x+i), c(y+j), c(z+k)), i, j, k in {-1, 0, 1}:
 * integer formats by value, R16F by the IEEE totalOrder of the stored halves (key = bits ^ (bits & 0x8000 ? 0xFFFF : 0x8000) as u16).
 * The chosen texel is stored unchanged: a selection.  radius and weights are ignored.
 * Output.  dense_out (may be NULL): host memory of nx ny nz elements of the volume's format, x fastest; the call blocks, like
 * vk_volume_histogram.  VK_FILTER_INSTALL: the result replaces the context's volume, re-laid out in the layout vk_volume_info reports
 * now; census and skip maps are rebuilt under the (isosurface | projection, table) state in force; table, projection, isosurface,
 * lighting, shadows and clip box stay in force exactly as across vk_volume_upload_device; frames in flight drain and batches are
 * invalidated.  Without VK_FILTER_INSTALL no context state changes: no surface, counter, slot or map is touched.
 * The call runs on the context's current stream (inside vk_frame_begin / _end: that frame's) and allocates and frees its own buffers.
 * VK_ERR_INVALID, decided before any launch, outputs untouched: a NULL request, an unknown op or flag, a radius above
 * VK_FILTER_MAX_RADIUS, a used weight that is not finite or beyond +-VK_FILTER_MAX_WEIGHT, neither dense_out nor VK_FILTER_INSTALL,
 * VK_FILTER_INSTALL while a frame is being recorded, no volume.  VK_ERR_UNSUPPORTED ("filter: ..."): a BRICKED / QUADS / STAGED or
 * RGBA16F_PAIR volume -- the set the histogram and the mesh refuse.  VK_ERR_OOM: a buffer cannot be allocated; the old volume stays.
 * vk_filter_gaussian is host arithmetic and needs no context: g[k] = exp(-(k - r)^2 / (2 sigma^2)) in double, each divided by their
 * double sum (added in the order of k) and rounded once to f32.  VK_ERR_INVALID: sigma not finite or <= 0, radius outside
 * 1 .. VK_FILTER_MAX_RADIUS, NULL weights (its message is read with vk_last_error(NULL)). */
#define VK_FILTER_MAX_RADIUS 6
#define VK_FILTER_MAX_WEIGHT 1024.0f
enum { VK_FILTER_CONVOLVE = 0, VK_FILTER_MEDIAN3 = 1 };
enum { VK_FILTER_INSTALL = 1 };
struct vk_volume_filter {  /* no typedef: the function below bears the same name, so the type is always `struct vk_volume_filter` */
    int32_t  op;                                       /* VK_FILTER_CONVOLVE / _MEDIAN3 */
    uint32_t flags;                                    /* VK_FILTER_INSTALL */
    uint32_t radius[3];                                /* CONVOLVE: taps 2 r + 1 per axis (x, y, z); 0: the axis is skipped */
    float    weights[3][2 * VK_FILTER_MAX_RADIUS + 1]; /* CONVOLVE: w[axis][0 .. 2 r]; entries beyond 2 r are ignored */
};  /* 176 bytes */
int vk_volume_filter(vk_ctx *ctx, const struct vk_volume_filter *f, void *dense_out);
int vk_filter_gaussian(double sigma_voxels, uint32_t radius, float *weights /* 2 radius + 1 */);

/* Connected components of a value range: the voxels whose stored texel lies in [lo, hi] are labelled by component,
 * and components are kept or dropped -- "only the largest connected thing above 0.3", "nothing smaller than 500 voxels", "the thing under
 * this pixel" -- so that the mesh, the histogram and every march see the cleaned volume without a round trip through the host.  Every
 * result is an integer or a stored texel: there is no rounding anywhere but in the fill.
 * Foreground.  t is the STORED texel as f32 on the kernel's scale (R8 0..255, R16_UNORM 0..65535, R16F the value).  lo_k and hi_k are
 * formed from lo and hi exactly as vk_set_isosurface forms iso_k: lo * 255.0f, lo * 65535.0f, or lo.  A voxel is foreground iff it lies
 * in the voxel box and t >= lo_k && t <= hi_k: a NaN never is, an R16F infinity is when the range reaches it.  The box is
 * vk_volume_histogram's: `box`, the clip box under VK_LABEL_CLIP_BOX (box must then be NULL), or NULL for the whole volume; an empty
 * box means no foreground.
 * Neighbours.  Two foreground voxels are adjacent when their index difference d has max |d_c| = 1 and sum |d_c| <= 1 (connectivity
 * 6), <= 2 (18) or <= 3 (26).  No wrap and no clamping at the volume's or the box's edge.  A component is a class of the transitive
 * closure of adjacency.
 * Numbering.  `first` of a component is its smallest linear index x + nx (y + ny z).  Components are numbered 1 .. n by increasing
 * first: raster order of first encounter.  labels_out (may be NULL): nx ny nz uint32, x fastest, over the whole volume; 0 is background,
 * which includes every voxel outside the box.  components (may be NULL): the first min(n, cap_components) entries in id order, each
 * n_voxels, first and the tight half-open bounding box.  result (may be NULL): n_components, n_foreground (the voxels of all
 * components), n_kept_components, n_kept_voxels.  The output is bit for bit the same on every layout, launch shape and run.
 * Selection.  VK_LABEL_KEEP_ALL: every component.  _KEEP_LARGEST: the first min(count, n) components in the order
 * n_voxels descending, then first ascending.  _KEEP_MIN_SIZE: the components with n_voxels >= count.  _KEEP_SEEDS: the components that contain
 * one of the seeds[0 .. n_seeds) voxels; a seed on background (also: outside the box) selects nothing.  M(v) holds iff v belongs to a
 * selected component.  The output texel is M(v) ? the stored bits unchanged : F; under VK_LABEL_INVERT it is M(v) ? F : stored.  F is
 * `fill` through vk_volume_filter's store rule: R8 (uint8) rintf(fminf(fmaxf(fill * 255.0f, 0.0f), 255.0f)), ties to even;
 * R16_UNORM the same with 65535; R16F round to nearest even.  (PACKED_PAIRS: the stored texel is the u8 value tap + delta.)
 * n_kept_components and n_kept_voxels count the selected components and their voxels, inverted or not.
 * Output and state.  dense_out (may be NULL; host memory of nx ny nz elements of the volume's format) and VK_LABEL_INSTALL behave
 * exactly as vk_volume_filter's dense_out and VK_FILTER_INSTALL: the same re-layout, the same state kept in force, the old volume
 * stays on any failure.  Without VK_LABEL_INSTALL no context state changes.  The call blocks, runs on the context's current stream
 * and allocates and frees its own buffers.
 * VK_ERR_INVALID, decided before any launch, outputs untouched: a NULL request; lo or hi NaN, lo > hi, a fill that is not finite; a
 * connectivity other than 6, 18, 26; an unknown flag or keep value; pad != 0; count or n_seeds that does not fit the keep mode (see the
 * struct); a seed outside the volume; components != NULL with cap_components == 0; none of labels_out, components, dense_out,
 * VK_LABEL_INSTALL and result requested; VK_LABEL_INSTALL while a frame is being recorded; a box that is inverted or leaves the
 * volume, a box together with VK_LABEL_CLIP_BOX; no volume.  VK_ERR_UNSUPPORTED ("label: ..."): a BRICKED / QUADS / STAGED or
 * RGBA16F_PAIR volume; a volume of more than 2^32 - 2 voxels (labels are 32-bit).  VK_ERR_OOM: a buffer cannot be allocated.
 * "Outputs untouched" holds for these refusals.  A call that fails later -- an allocation, a launch, or under VK_LABEL_INSTALL the
 * re-layout of the result, which runs last -- may have written labels_out, components, dense_out and *result already; the context's
 * volume is the old one whenever the call does not return VK_OK. */
#define VK_LABEL_MAX_SEEDS 16
enum { VK_LABEL_KEEP_ALL = 0, VK_LABEL_KEEP_LARGEST = 1, VK_LABEL_KEEP_MIN_SIZE = 2, VK_LABEL_KEEP_SEEDS = 3 };
enum { VK_LABEL_CLIP_BOX = 1, VK_LABEL_INSTALL = 2, VK_LABEL_INVERT = 4 };
typedef struct vk_label_request {
    float    lo, hi;          /* sample values, like vk_isosurface.iso; -inf / +inf allowed, NaN and lo > hi refused */
    uint32_t connectivity;    /* 6, 18 or 26 */
    uint32_t flags;           /* VK_LABEL_CLIP_BOX | VK_LABEL_INSTALL | VK_LABEL_INVERT */
    int32_t  keep;            /* VK_LABEL_KEEP_* */
    uint32_t n_seeds;         /* KEEP_SEEDS: 1 .. VK_LABEL_MAX_SEEDS; otherwise 0 */
    uint64_t count;           /* KEEP_LARGEST: how many (>= 1); KEEP_MIN_SIZE: the least number of voxels (>= 1); otherwise 0 */
    float    fill;            /* sample value that replaces a voxel that is not kept; finite */
    uint32_t pad;             /* 0 */
    uint32_t seeds[VK_LABEL_MAX_SEEDS][3];   /* voxel indices x, y, z, inside the volume */
} vk_label_request;           /* 232 bytes */
typedef struct vk_component {
    uint64_t n_voxels, first;
    vk_voxel_box box;         /* tight, half-open */
} vk_component;               /* 40 bytes */
typedef struct vk_label_result {
    uint64_t n_components, n_foreground, n_kept_components, n_kept_voxels;
} vk_label_result;            /* 32 bytes */
int vk_label_components(vk_ctx *ctx, const vk_label_request *req, const vk_voxel_box *box, uint32_t *labels_out, vk_component *components,
                        uint64_t cap_components, void *dense_out, vk_label_result *result);

/* Exact Euclidean distance transform of a value range, and morphology by a radius: how far every voxel is from
 * the set S of voxels whose stored texel lies in [lo, hi], as a squared distance over integer spacings -- an integer -- and the four
 * operations built on it: grow, shrink, close and open S by a Euclidean ball.  Every result is an integer or a stored texel: there is
 * no rounding anywhere but in the two fills.
 * The set S is exactly vk_label_components' foreground: t, lo_k and hi_k as there; a voxel is in S iff it lies in the voxel box and
 * t >= lo_k && t <= hi_k.  A NaN never is.  The box is `box`, the clip box under VK_DIST_CLIP_BOX (box must then be NULL), or NULL for
 * the whole volume.  The box restricts S only: the transform and every output cover the whole volume, and not S means every voxel of
 * the volume that is not in S, inside the box or outside it.
 * Distance.  For a set A of voxels of the volume, D2(A, v) = min over u in A of sum_c (spacing[c] * (v_c - u_c))^2 with c over x, y, z,
 * and D2(A, v) = VK_DIST_INF when A is empty.  Only voxels of the volume are candidates: nothing outside the volume is foreground or
 * background.  The call returns VK_ERR_UNSUPPORTED before any launch when sum_c (spacing[c] * (n_c - 1))^2 > 0xFFFFFFFE, so every
 * finite D2 fits in 32 bits and is never VK_DIST_INF.
 * Distance ops.  VK_DIST_OUTSIDE: d2_out[v] = D2(S, v), 0 on S.  VK_DIST_INSIDE: d2_out[v] = D2(not S, v), 0 off S.  d2_out (may be
 * NULL): nx ny nz uint32, x fastest.
 * Morphology ops.  R2 = (uint64_t)floor((double)radius * (double)radius).  dil(A) = { v : D2(A, v) <= R2 };
 * ero(A) = { v : D2(not A, v) > R2 }.  VK_DIST_DILATE: M = dil(S).  _ERODE: M = ero(S).  _CLOSE: M = ero(dil(S)).  _OPEN:
 * M = dil(ero(S)).  VK_DIST_INF is never <= R2: the empty set dilates to the empty set, the full volume erodes to the full volume.
 * Output texel.  A voxel in M and not in S becomes fill_in, a voxel in S and not in M becomes fill_out, each through
 * vk_label_components' fill rule F; every other voxel keeps its stored bits unchanged (PACKED_PAIRS: the u8 value tap + delta).
 * dense_out (may be NULL; host memory of nx ny nz elements of the volume's format) and VK_DIST_INSTALL behave exactly as
 * vk_label_components' dense_out and VK_LABEL_INSTALL: the same re-layout, the same state kept in force, the old volume stays on any
 * failure.  Without VK_DIST_INSTALL no context state changes.  The call blocks, runs on the context's current stream and allocates and
 * frees its own buffers.
 * result (may be NULL).  n_foreground = |S|.  Morphology ops: n_result = |M|, n_added = |M \ S|, n_removed = |S \ M|, max_d2 = 0.
 * Distance ops: n_result = n_foreground, n_added = n_removed = 0, max_d2 = the largest d2_out that is not VK_DIST_INF (0 if none).
 * VK_ERR_INVALID, decided before any launch, outputs untouched: a NULL request; lo or hi NaN, lo > hi; an unknown op or flag; a
 * spacing of 0 or above VK_DIST_MAX_SPACING; a radius that is not finite, is negative or lies above VK_DIST_MAX_RADIUS; a nonzero
 * radius with a distance op; a fill that is not finite; d2_out with a morphology op; dense_out or VK_DIST_INSTALL with a distance op;
 * nothing requested (distance op: neither d2_out nor result; morphology op: none of dense_out, VK_DIST_INSTALL and result);
 * VK_DIST_INSTALL while a frame is being recorded; a box that is inverted or leaves the volume, a box together with
 * VK_DIST_CLIP_BOX; no volume.  VK_ERR_UNSUPPORTED ("distance: ..."): a BRICKED / QUADS / STAGED or RGBA16F_PAIR volume; a volume of
 * more than 2^32 - 2 voxels; the overflow condition above.  VK_ERR_OOM: a buffer cannot be allocated.  A call that fails later may
 * have written its outputs already; the context's volume is the old one whenever the call does not return VK_OK. */
#define VK_DIST_INF         0xFFFFFFFFu
#define VK_DIST_MAX_SPACING 64
#define VK_DIST_MAX_RADIUS  65535.0f
enum { VK_DIST_OUTSIDE = 0, VK_DIST_INSIDE = 1, VK_DIST_DILATE = 2, VK_DIST_ERODE = 3, VK_DIST_CLOSE = 4, VK_DIST_OPEN = 5 };
enum { VK_DIST_CLIP_BOX = 1, VK_DIST_INSTALL = 2 };
typedef struct vk_distance_request {
    float    lo, hi;         /* the value range, formed exactly as vk_label_components forms lo_k, hi_k */
    int32_t  op;             /* VK_DIST_OUTSIDE .. VK_DIST_OPEN */
    uint32_t flags;          /* VK_DIST_CLIP_BOX | VK_DIST_INSTALL */
    uint32_t spacing[3];     /* integer voxel pitch per axis x, y, z: 1 .. VK_DIST_MAX_SPACING */
    float    radius;         /* DILATE .. OPEN: in the units of spacing; otherwise 0 */
    float    fill_in;        /* sample value of a voxel that joins the set; finite */
    float    fill_out;       /* sample value of a voxel that leaves it; finite */
} vk_distance_request;       /* 40 bytes */
typedef struct vk_distance_result {
    uint64_t n_foreground, n_result, n_added, n_removed;
    uint32_t max_d2;         /* OUTSIDE / INSIDE: the largest D2 that is not VK_DIST_INF (0 if none); otherwise 0 */
    uint32_t pad;
} vk_distance_result;        /* 40 bytes */
#ifdef __cplusplus
static_assert(sizeof(vk_distance_request) == 40 && sizeof(vk_distance_result) == 40, "vk_distance_request, vk_distance_result: 40 bytes each");
#else
_Static_assert(sizeof(vk_distance_request) == 40 && sizeof(vk_distance_result) == 40, "vk_distance_request, vk_distance_result: 40 bytes each");
#endif
int vk_distance_transform(vk_ctx *ctx, const vk_distance_request *req, const vk_voxel_box *box, uint32_t *d2_out, void *dense_out,
                          vk_distance_result *result);

/* Split touching objects: the set S of voxels whose stored texel lies in [lo, hi] is eroded by a radius, what
 * survives is labelled as markers, the markers grow back over S -- every voxel joins the marker that reaches it first -- and S is cut
 * where two regions meet, so that vk_label_components, the keep modes and the mesh see separate objects afterwards.  Every result is
 * an integer or a stored texel: there is no rounding anywhere but in the fill.
 * Foreground.  S, t, lo_k, hi_k and the box are exactly vk_distance_transform's: a voxel is in S iff it lies in the voxel box (`box`,
 * the clip box under VK_SPLIT_CLIP_BOX, or NULL for the whole volume) and t >= lo_k && t <= hi_k.  The box restricts S only.
 * Adjacency.  connectivity is 6, 18 or 26, exactly as in vk_label_components: two voxels are adjacent when their index difference d
 * has max |d_c| = 1 and sum |d_c| <= 1, 2 or 3.  No wrap and no clamping.
 * Markers.  R2 = (uint64_t)floor((double)radius * (double)radius).  K = ero(S) = { v in S : D2(not S, v) > R2 }, with D2 over the
 * integer `spacing` exactly as VK_DIST_ERODE.  VK_DIST_INF > R2 always holds, so when S is the whole volume K = S.  The marker
 * components are the components of K under `connectivity`.
 * Steps.  g(v) = 0 on K.  For v in S \ K, g(v) is the least k for which a path v0 in K, v1, ..., vk = v exists whose every vi lies in
 * S and whose consecutive voxels are adjacent.  A voxel of S with no such path is unreached; a component of S is unreached either as
 * a whole or not at all.
 * Anchors and regions.  A marker component's anchor is its smallest linear index x + nx (y + ny z).  a(v) on K is the anchor of v's
 * marker component.  For a reached v with g(v) = k > 0: a(v) = min { a(u) : u in S, u adjacent to v, g(u) = k - 1 }.  The unreached
 * voxels are labelled as vk_label_components would label them: components under `connectivity`, each with its smallest linear index
 * as anchor.  A region is the set of voxels that share one a.  Regions are numbered 1 .. N by increasing anchor; marker regions and
 * unreached (residue) regions share this one numbering.  radius = 0, or any radius that leaves K empty, gives bit for bit
 * vk_label_components' labels and table; every region is connected under `connectivity`; the result depends on no launch shape,
 * schedule or layout.
 * Outputs.  labels_out (may be NULL): nx ny nz uint32, x fastest, 0 off S.  components (may be NULL): the first
 * min(N, cap_components) regions in id order; `first` is the region's ANCHOR -- a grown region can hold smaller indices than its
 * anchor -- and n_voxels and box cover the whole region.  result (may be NULL): n_regions = N, n_foreground = |S|, n_markers (the
 * marker components), n_marker_voxels = |K|, n_residue_regions and n_residue_voxels (the unreached regions and their voxels), n_cut,
 * and rounds: the largest finite g, or 0 if there is none -- defined by the rule, not by the implementation.
 * Cut.  A voxel v of S is cut iff some adjacent u in S lies in a region with a smaller id.  The output texel of a cut voxel is
 * fill_out through vk_label_components' fill rule F; every other voxel keeps its stored bits.  Only the later region's side is cut,
 * so the cut is one voxel thick; afterwards no two adjacent voxels of S that were not cut lie in different regions.  dense_out (may be
 * NULL) and VK_SPLIT_INSTALL behave exactly as vk_label_components' dense_out and VK_LABEL_INSTALL.  The call blocks, runs on the
 * context's current stream and allocates and frees its own buffers.
 * VK_ERR_INVALID, decided before any launch, outputs untouched ("vk_split_components: ..."): a NULL request; lo or hi NaN,
 * lo > hi; a connectivity other than 6, 18, 26; an unknown flag; pad != 0; a spacing of 0 or above VK_DIST_MAX_SPACING; a radius that
 * is not finite, is negative or lies above VK_DIST_MAX_RADIUS; a fill_out that is not finite; components != NULL with
 * cap_components == 0; none of labels_out, components, dense_out, VK_SPLIT_INSTALL and result requested; with dense_out or
 * VK_SPLIT_INSTALL an F(fill_out) whose value on the kernel's scale lies inside [lo_k, hi_k] (such a cut would cut nothing);
 * VK_SPLIT_INSTALL while a frame is being recorded; a box that is inverted or leaves the volume, a box together with
 * VK_SPLIT_CLIP_BOX; no volume.  VK_ERR_UNSUPPORTED ("split: ..."): a BRICKED / QUADS / STAGED or RGBA16F_PAIR volume; a volume of
 * more than 2^32 - 2 voxels; sum_c (spacing[c] * (n_c - 1))^2 > 0xFFFFFFFE.  VK_ERR_OOM: a buffer cannot be allocated.  A call that
 * fails later may have written its outputs already; the context's volume is the old one whenever the call does not return VK_OK. */
enum { VK_SPLIT_CLIP_BOX = 1, VK_SPLIT_INSTALL = 2 };
typedef struct vk_split_request {
    float    lo, hi;         /* the value range, formed exactly as vk_label_components forms lo_k, hi_k */
    uint32_t connectivity;   /* 6, 18 or 26 */
    uint32_t flags;          /* VK_SPLIT_CLIP_BOX | VK_SPLIT_INSTALL */
    uint32_t spacing[3];     /* integer voxel pitch per axis x, y, z: 1 .. VK_DIST_MAX_SPACING */
    float    radius;         /* the erosion radius in the units of spacing: 0 .. VK_DIST_MAX_RADIUS */
    float    fill_out;       /* sample value of a cut voxel; finite, outside [lo, hi] once stored */
    uint32_t pad;            /* 0 */
} vk_split_request;          /* 40 bytes */
typedef struct vk_split_result {
    uint64_t n_regions, n_foreground, n_markers, n_marker_voxels, n_residue_regions, n_residue_voxels, n_cut;
    uint32_t rounds;         /* the largest finite g (0: none) */
    uint32_t pad;
} vk_split_result;           /* 64 bytes */
#ifdef __cplusplus
static_assert(sizeof(vk_split_request) == 40 && sizeof(vk_split_result) == 64, "vk_split_request: 40 bytes, vk_split_result: 64 bytes");
#else
_Static_assert(sizeof(vk_split_request) == 40 && sizeof(vk_split_result) == 64, "vk_split_request: 40 bytes, vk_split_result: 64 bytes");
#endif
int vk_split_components(vk_ctx *ctx, const vk_split_request *req, const vk_voxel_box *box, uint32_t *labels_out, vk_component *components,
                        uint64_t cap_components, void *dense_out, vk_split_result *result);

/* Measure labelled regions: the volume and a label array are reduced into one exact integer record per region --
 * voxel count, first voxel, box, the sums of the voxel indices and of their products, the sums of the stored texel and of its square,
 * its extremes, and the exposed voxel faces per axis.  Every field is an integer; the hosts derive centroid, covariance, principal
 * axes, mean, deviation, volume and surface from it.
 * Labels.  labels_in == NULL: the regions are vk_label_components' components of [lo, hi] under `connectivity` inside the voxel box
 * (`box`, the clip box under VK_MEASURE_CLIP_BOX, or NULL for the whole volume), numbered as there; the label array stays on the
 * device.  After a VK_SPLIT_INSTALL these are the split regions, since the cut separates them.  labels_in != NULL: a host array of
 * nx ny nz uint32, x fastest, 0 background -- vk_label_components' or vk_split_components' labels_out, or a caller's segmentation;
 * the regions are the ids 1 .. max_label; lo, hi and connectivity must be 0, box NULL and VK_MEASURE_CLIP_BOX clear.  An id above
 * max_label is found on the device after the upload and refused (VK_ERR_INVALID, outputs untouched).  An id no voxel carries gives a
 * record with n_voxels = 0, first = UINT64_MAX, a box of zeros, q_min = INT64_MAX, q_max = INT64_MIN and zero sums.
 * q.  q(v) is the stored texel of voxel v on an integer scale: R8 and R16_UNORM the stored integer, R16F t 2^24 (every finite half is a
 * multiple of 2^-24; |q| < 2^40; -0 gives 0), PACKED_PAIRS the value tap.  result->scale is the divisor from q to the sample value:
 * 255, 65535 or 16777216.
 * The record.  n_voxels, first (the smallest linear index x + nx (y + ny z)) and box (tight, half-open) as vk_component.  sum_x ..
 * sum_yz: the sums over the region's voxels of x, y, z, x x, y y, z z, x y, x z, y z.  n_nonfinite: the voxels whose texel is NaN or
 * +-inf (R16F; 0 otherwise); they are left out of q_min, q_max, sum_q and sum_qq.  sum_q = sum_q_hi 2^64 + sum_q_lo is a signed
 * 128-bit two's complement sum of q, sum_qq = sum_qq_hi 2^64 + sum_qq_lo the unsigned 128-bit sum of q q: both exact.  faces[a]: for
 * each voxel of the region and each of its two neighbours along axis a (x, y, z), one when the neighbour lies outside the volume or
 * carries another label (background and everything outside the box are label 0); a face between two regions counts once for each.
 * Outputs.  regions (may be NULL): the first min(n_regions, cap_regions) records in id order.  result (may be NULL): n_regions (the
 * components found, or max_label), n_foreground (the voxels with a label), records_written, scale.  No context state changes: the
 * call is allowed while a frame is being recorded.  It blocks, runs on the context's current stream and frees its buffers.  The
 * records depend on no launch shape, schedule or layout.
 * VK_ERR_INVALID, decided before any launch, outputs untouched ("vk_measure_components: ..."): a NULL request; lo or hi NaN, lo > hi;
 * without labels_in a connectivity other than 6, 18, 26; an unknown flag; pad != 0; regions != NULL with cap_regions == 0; neither
 * regions nor result requested; with labels_in a nonzero lo, hi or connectivity, a box or VK_MEASURE_CLIP_BOX, max_label == 0;
 * without labels_in max_label != 0; no volume; a box that is inverted or leaves the volume, a box together with
 * VK_MEASURE_CLIP_BOX; max_label above the voxel count.  VK_ERR_UNSUPPORTED ("measure: ..."): a BRICKED / QUADS / STAGED or
 * RGBA16F_PAIR volume; a volume of more than 2^32 - 2 voxels; a volume whose n (max dimension - 1)^2 does not fit 64 bits (an index
 * sum could overflow).  VK_ERR_OOM: a buffer cannot be allocated. */
enum { VK_MEASURE_CLIP_BOX = 1 };
typedef struct vk_measure_request {
    float    lo, hi;         /* the value range, formed exactly as vk_label_components forms lo_k, hi_k; 0 with labels_in */
    uint32_t connectivity;   /* 6, 18 or 26; 0 with labels_in */
    uint32_t flags;          /* VK_MEASURE_CLIP_BOX */
    uint32_t max_label;      /* with labels_in: the regions are 1 .. max_label; otherwise 0 */
    uint32_t pad;            /* 0 */
} vk_measure_request;        /* 24 bytes */
typedef struct vk_region {
    uint64_t n_voxels, first;
    vk_voxel_box box;        /* tight, half-open; zeros for an empty region */
    uint64_t sum_x, sum_y, sum_z;
    uint64_t sum_xx, sum_yy, sum_zz, sum_xy, sum_xz, sum_yz;
    uint64_t n_nonfinite;
    int64_t  q_min, q_max;   /* over the finite voxels; INT64_MAX / INT64_MIN when there are none */
    int64_t  sum_q_hi;       /* signed 128-bit: sum_q_hi 2^64 + sum_q_lo */
    uint64_t sum_q_lo;
    uint64_t sum_qq_hi, sum_qq_lo;  /* unsigned 128-bit */
    uint64_t faces[3];       /* exposed voxel faces across x, y, z */
} vk_region;                 /* 192 bytes */
typedef struct vk_measure_result {
    uint64_t n_regions, n_foreground, records_written;
    uint32_t scale;          /* 255, 65535 or 16777216 */
    uint32_t pad;
} vk_measure_result;         /* 32 bytes */
#ifdef __cplusplus
static_assert(sizeof(vk_measure_request) == 24 && sizeof(vk_region) == 192 && sizeof(vk_measure_result) == 32, "vk_measure_request: 24 bytes, vk_region: 192, vk_measure_result: 32");
#else
_Static_assert(sizeof(vk_measure_request) == 24 && sizeof(vk_region) == 192 && sizeof(vk_measure_result) == 32, "vk_measure_request: 24 bytes, vk_region: 192, vk_measure_result: 32");
#endif
int vk_measure_components(vk_ctx *ctx, const vk_measure_request *req, const vk_voxel_box *box, const uint32_t *labels_in, vk_region *regions,
                          uint64_t cap_regions, vk_measure_result *result);

/* Local thickness of a value range: for every voxel of the set S, the squared radius of the largest ball that
 * fits inside S and contains the voxel -- trabecular thickness, strut thickness, pore size.  Every result is an integer but the dense
 * value, whose three roundings are written out below.
 * The set.  S, t, lo_k, hi_k, the box (`box`, the clip box under VK_THICK_CLIP_BOX, or NULL for the whole volume) and the integer
 * `spacing` are exactly vk_distance_transform's.  The box restricts S only.
 * Distances.  d2(u, v) = sum_c (spacing[c] * (u_c - v_c))^2.  D(u) = D2(not S, u) as VK_DIST_INSIDE defines it: 0 off S, and
 * VK_DIST_INF on S when S is the whole volume -- nothing outside the volume is background.
 * The cap.  C = (uint64_t)floor((double)max_radius * (double)max_radius); Dc(u) = min(D(u), C).  The cap bounds the reach of every
 * ball and with it the work of a launch, and it saturates the result: a structure thicker than max_radius reports C.  VK_DIST_INF
 * never appears in an output.
 * Thickness.  For v in S: T2(v) = max { Dc(u) : u in S, d2(u, v) < Dc(u) }.  For v not in S: T2(v) = 0.  The ball is open: the set of
 * w with d2(u, w) < D(u) is the largest ball about u that holds no background voxel.  u = v always qualifies, so T2 >= Dc > 0 on S.
 * The thickness a user reads is 2 sqrt(T2), in the units of spacing; the hosts derive it.
 * Outputs.  t2_out (may be NULL): nx ny nz uint32, x fastest, over the whole volume.  The dense value of v in S is
 * w(v) = sqrtf((float)T2(v)) * gain: the conversion (exact: T2 <= 2^22), the correctly rounded square root and the product are each
 * rounded once, nothing is fused; it is stored through vk_label_components' fill rule F.  A voxel outside S stores F(fill_out).
 * gain == 0 asks for the automatic gain 1.0f / sqrtf((float)max_t2), or 0 when max_t2 is 0: the thickest place stores full scale.
 * dense_out (may be NULL; host memory of nx ny nz elements of the volume's format) and VK_THICK_INSTALL behave exactly as
 * vk_distance_transform's dense_out and VK_DIST_INSTALL: the same re-layout, the table, projection, isosurface, lighting and clip box
 * stay in force, the old volume stays on any failure.  Without VK_THICK_INSTALL no context state changes.  The call blocks, runs on
 * the context's current stream and allocates and frees its own buffers.
 * result (may be NULL).  n_foreground = |S|; max_t2 = the largest T2 (0: S is empty); n_saturated = the voxels with T2 == C; sum_t2
 * = the sum of T2 over S; gain = the gain used.  sum_t2 cannot overflow: C <= (VK_THICK_MAX_REACH * VK_DIST_MAX_SPACING)^2 = 2^22 and
 * |S| < 2^32, so the sum stays below 2^54.
 * VK_ERR_INVALID, decided before any launch, outputs untouched ("vk_local_thickness: ..."), in this order: a NULL request; lo or hi
 * NaN; lo > hi; an unknown flag; a spacing of 0 or above VK_DIST_MAX_SPACING; a max_radius that is not finite or lies below 1;
 * max_radius / min_c spacing[c] > VK_THICK_MAX_REACH (the largest ball then reaches no further than 32 voxels along any axis, which
 * keeps the window a tile of 8^3 voxels gathers from at (8 + 64)^3 voxels); a gain that is negative or not finite; a fill_out that
 * is not finite; none of t2_out, dense_out, VK_THICK_INSTALL and result requested; then VK_THICK_INSTALL while a frame is being
 * recorded; no volume; a box that is inverted or leaves the volume, a box together with VK_THICK_CLIP_BOX.  VK_ERR_UNSUPPORTED
 * ("thickness: ..."): a BRICKED / QUADS / STAGED or RGBA16F_PAIR volume; a volume of more than 2^32 - 2 voxels;
 * sum_c (spacing[c] * (n_c - 1))^2 > 0xFFFFFFFE.  VK_ERR_OOM: a buffer cannot be allocated.  A call that fails later may have written
 * its outputs already; the context's volume is the old one whenever the call does not return VK_OK. */
#define VK_THICK_MAX_REACH 32
enum { VK_THICK_CLIP_BOX = 1, VK_THICK_INSTALL = 2 };
typedef struct vk_thickness_request {
    float    lo, hi;         /* the value range, formed exactly as vk_label_components forms lo_k, hi_k */
    uint32_t flags;          /* VK_THICK_CLIP_BOX | VK_THICK_INSTALL */
    uint32_t spacing[3];     /* integer voxel pitch per axis x, y, z: 1 .. VK_DIST_MAX_SPACING */
    float    max_radius;     /* the cap, in the units of spacing: >= 1, at most VK_THICK_MAX_REACH times the smallest spacing */
    float    gain;           /* the dense value is sqrtf(T2) * gain; 0: 1 / sqrtf(max_t2) */
    float    fill_out;       /* sample value of a voxel outside S; finite */
} vk_thickness_request;      /* 36 bytes */
typedef struct vk_thickness_result {
    uint64_t n_foreground, n_saturated, sum_t2;
    uint32_t max_t2;         /* the largest T2 (0: S is empty) */
    float    gain;           /* the gain used */
} vk_thickness_result;       /* 32 bytes */
#ifdef __cplusplus
static_assert(sizeof(vk_thickness_request) == 36 && sizeof(vk_thickness_result) == 32, "vk_thickness_request: 36 bytes, vk_thickness_result: 32 bytes");
#else
_Static_assert(sizeof(vk_thickness_request) == 36 && sizeof(vk_thickness_result) == 32, "vk_thickness_request: 36 bytes, vk_thickness_result: 32 bytes");
#endif
int vk_local_thickness(vk_ctx *ctx, const vk_thickness_request *req, const vk_voxel_box *box, uint32_t *t2_out, void *dense_out,
                       vk_thickness_result *result);

/* Geodesic distance through a value range: for every voxel of the set S, the length of the shortest path that
 * stays inside S, from a face of the box or from picked voxels -- percolation, tortuosity, the reachable fraction.  Every result is
 * an integer but the dense value, whose two roundings are written out below.
 * The set.  S, t, lo_k, hi_k and the integer `spacing` are exactly vk_distance_transform's.  The box B is `box`, the clip box under
 * VK_GEO_CLIP_BOX, or the whole volume (NULL).  A voxel is in S iff it lies in B and t >= lo_k && t <= hi_k.  B restricts S; the
 * outputs cover the whole volume.
 * Adjacency.  connectivity is 6, 18 or 26, exactly as in vk_label_components: no wrap, no clamping.
 * Step cost.  For an adjacent pair with index difference d: q(d) = sum_c (spacing[c] * d_c)^2, 1 <= q <= 12288, and w(d) is the
 * largest integer r with r * r <= q * 65536 -- the floor of 256 sqrt(q), computed in integers.  At spacing (1,1,1) the costs are 256,
 * 362 and 443, at (64,64,64) 16384, 23170 and 28377, at (1,2,3) {256, 512, 572, 768, 809, 923, 957}.  One unit (VK_GEO_UNIT) is 1/256
 * of a spacing unit.
 * Sources.  source_faces is a mask of six bits: 1 x-, 2 x+, 4 y-, 8 y+, 16 z-, 32 z+.  A voxel of S lies on a face when its
 * coordinate equals B's first or last index on that axis.  seeds[0 .. n_seeds) are voxel indices inside the volume.  The source set
 * is A = S n (faces u seeds); a seed off S contributes nothing, as in VK_LABEL_KEEP_SEEDS.
 * Distance.  g(v) = 0 on A.  For other v in S, g(v) = min(L(v), VK_GEO_FAR), L(v) the least sum of step costs over paths
 * v0 in A, ..., vk = v whose every voxel lies in S and whose consecutive voxels are adjacent.  g(v) = VK_GEO_INF where there is no
 * such path, and off S.  Every relaxation is the saturating min(a + w, VK_GEO_FAR) of a finite a: saturation is monotone and
 * commutes with min, so g is the unique fixed point and depends on no order, launch shape or layout.
 * Targets.  target_faces is a second face mask and may be 0.  target_min is the least g over the voxels of S on those faces,
 * VK_GEO_INF when no such voxel is reached or the mask is 0; n_target_reached counts the reached voxels among them.
 * Outputs.  g_out (may be NULL): nx ny nz uint32, x fastest.  The dense value of a reached voxel of S is (float)g(v) * gain: the
 * conversion rounds once to nearest even, the product rounds once, nothing is fused; an unreached voxel of S stores fill_unreached,
 * a voxel off S fill_out; all three go through vk_label_components' fill rule F.  gain == 0 asks for 1.0f / (float)max_g, or 0 when
 * max_g == 0.  dense_out (may be NULL; host memory of nx ny nz elements of the volume's format) and VK_GEO_INSTALL behave exactly as
 * vk_local_thickness' dense_out and VK_THICK_INSTALL: the same re-layout, the table, projection, isosurface, lighting and clip box
 * stay in force, the old volume stays on any failure.  Without VK_GEO_INSTALL no context state changes.  The call blocks, runs on
 * the context's current stream and allocates and frees its own buffers.
 * result (may be NULL).  n_foreground = |S|; n_sources = |A|; n_reached = the voxels of S with finite g, sources included;
 * n_saturated = those with g == VK_GEO_FAR; n_target_reached; sum_g = the sum of g over the reached voxels (below 2^64: fewer than
 * 2^32 voxels of less than 2^32 each); max_g = the largest finite g, 0 if none; target_min; gain = the gain used.  No field depends
 * on how many rounds the implementation took.
 * VK_ERR_INVALID, decided before any launch, outputs untouched ("vk_geodesic_distance: ..."), in this order: a NULL request; lo or
 * hi NaN; lo > hi; a connectivity other than 6, 18, 26; an unknown flag; pad != 0; a spacing of 0 or above VK_DIST_MAX_SPACING; a
 * face mask with a bit above 32; n_seeds > VK_GEO_MAX_SEEDS; source_faces == 0 && n_seeds == 0; a gain that is negative or not
 * finite; a fill_out or fill_unreached that is not finite; none of g_out, dense_out, VK_GEO_INSTALL and result requested; then
 * VK_GEO_INSTALL while a frame is being recorded; no volume; a seed outside the volume; a box that is inverted or leaves the volume,
 * a box together with VK_GEO_CLIP_BOX.  VK_ERR_UNSUPPORTED ("geodesic: ..."): a BRICKED / QUADS / STAGED or RGBA16F_PAIR volume; a
 * volume of more than 2^32 - 2 voxels.  VK_ERR_OOM: a buffer cannot be allocated.  A call that fails later may have written its
 * outputs already; the context's volume is the old one whenever the call does not return VK_OK. */
#define VK_GEO_INF 0xFFFFFFFFu
#define VK_GEO_FAR 0xFFFFFFFEu
#define VK_GEO_UNIT 256u
#define VK_GEO_MAX_SEEDS 16
enum { VK_GEO_CLIP_BOX = 1, VK_GEO_INSTALL = 2 };
enum { VK_GEO_FACE_X0 = 1, VK_GEO_FACE_X1 = 2, VK_GEO_FACE_Y0 = 4, VK_GEO_FACE_Y1 = 8, VK_GEO_FACE_Z0 = 16, VK_GEO_FACE_Z1 = 32 };
typedef struct vk_geodesic_request {
    float    lo, hi;                               /* the value range, formed exactly as vk_label_components forms lo_k, hi_k */
    uint32_t connectivity, flags;                  /* 6, 18 or 26; VK_GEO_CLIP_BOX | VK_GEO_INSTALL */
    uint32_t spacing[3];                           /* integer voxel pitch per axis x, y, z: 1 .. VK_DIST_MAX_SPACING */
    uint32_t source_faces, target_faces, n_seeds;  /* VK_GEO_FACE_* masks; the seeds in use */
    float    gain, fill_out, fill_unreached;       /* the dense value is (float)g * gain (0: 1 / max_g); the sample values off S and of an unreached voxel of S */
    uint32_t pad;                                  /* 0 */
    uint32_t seeds[VK_GEO_MAX_SEEDS][3];           /* voxel indices x, y, z */
} vk_geodesic_request;                             /* 248 bytes */
typedef struct vk_geodesic_result {
    uint64_t n_foreground, n_sources, n_reached, n_saturated, n_target_reached, sum_g;
    uint32_t max_g, target_min;
    float    gain;
    uint32_t pad;
} vk_geodesic_result;                              /* 64 bytes */
#ifdef __cplusplus
static_assert(sizeof(vk_geodesic_request) == 248 && sizeof(vk_geodesic_result) == 64, "vk_geodesic_request: 248 bytes, vk_geodesic_result: 64 bytes");
#else
_Static_assert(sizeof(vk_geodesic_request) == 248 && sizeof(vk_geodesic_result) == 64, "vk_geodesic_request: 248 bytes, vk_geodesic_result: 64 bytes");
#endif
int vk_geodesic_distance(vk_ctx *ctx, const vk_geodesic_request *req, const vk_voxel_box *box, uint32_t *g_out, void *dense_out,
                         vk_geodesic_result *result);

/* Skeleton of a value range: the set S thinned to a one-voxel-wide set K with the same pieces, tunnels and
 * cavities -- centre lines, from which follow free ends, branch points and centre-line length.  Every result is an integer.
 * The set.  S, t, lo_k, hi_k and the box B (`box`, the clip box under VK_SKEL_CLIP_BOX, or the whole volume) are exactly
 * vk_geodesic_distance's.  Everything not in S is background: voxels outside B, voxels outside the volume.  No wrap, no clamp.
 * Connectivity.  The set is 26-connected and the background 6-connected.  There is no other pairing.
 * Neighbourhood mask.  For a voxel v of the current set K, m(v) has bit k set iff the neighbour at offset o(k) is in K, with the
 * offsets numbered as vk_label_components numbers them, d = (o % 3 - 1, o / 3 % 3 - 1, o / 9 - 1), the centre (o = 13) skipped:
 * o(k) = k for k < 13 and k + 1 for k >= 13 -- 26 bits.
 * Simple point (Malandain and Bertrand).  skel_simple(m) is true iff both hold: (a) the set bits of m, joined by 26-adjacency among
 * the 26 positions, form exactly one component (zero components: not simple); (b) the clear bits among the 18 positions with
 * |d|_1 <= 2, joined by 6-adjacency among those 18 positions, have exactly one component that contains one of the 6 face positions.
 * Line end.  popcount(m) == 1.
 * Subfields.  sf(v) = (x & 1) | (y & 1) << 1 | (z & 1) << 2 on absolute voxel indices, not box-relative.  Two voxels of one subfield
 * are never 26-adjacent.
 * Iteration i = 1, 2, ...  Let K_i be the set at the iteration's start, K_1 = S.  The candidates C_i are the voxels of K_i with at
 * least one of the 6 face neighbours not in K_i; volume faces and B's faces therefore peel.  Then come eight sub-passes s = 0 .. 7 in
 * that order.  Sub-pass s looks at every voxel v with sf(v) == s, v in C_i, v still in K; in VK_SKEL_CURVE mode it also requires
 * that m(v) on the current K is not a line end; it deletes all such v with skel_simple(m(v)) at once.  The pass ends after the first
 * iteration that deletes nothing, or after max_iterations iterations if that is not 0.
 * Modes.  VK_SKEL_CURVE keeps line ends and gives centre lines.  VK_SKEL_KERNEL has no end condition and gives the ultimate homotopic
 * kernel: a blob becomes a voxel, a ring a closed curve, and a shell stays a closed surface.
 * Why the result depends on no launch shape, order or layout.  Within a sub-pass no deleted voxel lies in another deleted voxel's
 * N26: the simultaneous deletion equals a sequential one in any order, and each deletion is of a simple point.
 * Outputs.  class_out (may be NULL): nx ny nz bytes, x fastest: 0 off K, 1 isolated (0 neighbours in K), 2 end (1), 3 regular (2),
 * 4 junction (>= 3).  Dense value: a voxel of K keeps its stored bits (a PACKED_PAIRS voxel the u8 value tap + delta, as in
 * vk_morph_volume), or stores F(fill_in) under VK_SKEL_FILL_IN; every other voxel stores F(fill_out); F is vk_label_components' fill
 * rule.  dense_out (may be NULL) and VK_SKEL_INSTALL behave exactly as vk_geodesic_distance's dense_out and VK_GEO_INSTALL.  Without
 * VK_SKEL_INSTALL no context state changes.  The call blocks, runs on the context's current stream and allocates and frees its own
 * buffers.
 * result (may be NULL).  n_foreground = |S|; n_skeleton = |K|; n_isolated, n_end, n_regular, n_junction = the voxels of K per class;
 * links[j], j = 0 .. 12: the unordered 26-adjacent pairs of K whose offset is o = 14 + j (the offsets above the centre), so that the
 * hosts derive the length sum_j links[j] sqrt(q_j), q_j = sum_c (spacing[c] d_c)^2, for any spacing -- it counts every adjacent pair,
 * so it over-counts inside junction clumps, where voxels are adjacent to more than two others; iterations = the iterations that
 * deleted something; converged = 1 iff an iteration that deleted nothing ran (0: max_iterations stopped the pass first).
 * VK_ERR_INVALID, decided before any launch, outputs untouched ("vk_skeletonize: ..."), in this order: a NULL request; lo or hi NaN;
 * lo > hi; an unknown mode; an unknown flag; pad != 0; a fill_out that is not finite, or a fill_in that is not finite under
 * VK_SKEL_FILL_IN; none of class_out, dense_out, VK_SKEL_INSTALL and result requested; then VK_SKEL_INSTALL while a frame is being
 * recorded; no volume; a box that is inverted or leaves the volume, a box together with VK_SKEL_CLIP_BOX.  VK_ERR_UNSUPPORTED
 * ("skeleton: ..."): a BRICKED / QUADS / STAGED or RGBA16F_PAIR volume; a volume of more than 2^32 - 2 voxels.  VK_ERR_OOM: a buffer
 * cannot be allocated.  A call that fails later may have written its outputs already; the context's volume is the old one whenever
 * the call does not return VK_OK. */
enum { VK_SKEL_CURVE = 0, VK_SKEL_KERNEL = 1 };
enum { VK_SKEL_CLIP_BOX = 1, VK_SKEL_INSTALL = 2, VK_SKEL_FILL_IN = 4 };
enum { VK_SKEL_OFF = 0, VK_SKEL_ISOLATED = 1, VK_SKEL_END = 2, VK_SKEL_REGULAR = 3, VK_SKEL_JUNCTION = 4 };
#define VK_SKEL_LINKS 13
typedef struct vk_skeleton_request {
    float    lo, hi;                       /* the value range, formed exactly as vk_label_components forms lo_k, hi_k */
    uint32_t mode, flags;                  /* VK_SKEL_CURVE or VK_SKEL_KERNEL; VK_SKEL_CLIP_BOX | VK_SKEL_INSTALL | VK_SKEL_FILL_IN */
    uint32_t max_iterations;               /* 0: until an iteration deletes nothing */
    float    fill_in, fill_out;            /* the sample values of a voxel of K under VK_SKEL_FILL_IN, and of every other voxel */
    uint32_t pad;                          /* 0 */
} vk_skeleton_request;                     /* 32 bytes */
typedef struct vk_skeleton_result {
    uint64_t n_foreground, n_skeleton, n_isolated, n_end, n_regular, n_junction;
    uint64_t links[VK_SKEL_LINKS];
    uint32_t iterations, converged;
} vk_skeleton_result;                      /* 160 bytes */
#ifdef __cplusplus
static_assert(sizeof(vk_skeleton_request) == 32 && sizeof(vk_skeleton_result) == 160, "vk_skeleton_request: 32 bytes, vk_skeleton_result: 160 bytes");
#else
_Static_assert(sizeof(vk_skeleton_request) == 32 && sizeof(vk_skeleton_result) == 160, "vk_skeleton_request: 32 bytes, vk_skeleton_result: 160 bytes");
#endif
int vk_skeletonize(vk_ctx *ctx, const vk_skeleton_request *req, const vk_voxel_box *box, uint8_t *class_out, void *dense_out,
                   vk_skeleton_result *result);

/* Steady-state diffusion through a value range: the Laplace equation on the set S with no-flux walls,
 * concentration 1 on one face of the box and 0 on the opposite one -- the effective diffusivity ratio D_eff / D0 and the tortuosity
 * factor of a pore space.  The values are floats, and every one of them is defined bit for bit: a C loop that follows this comment
 * reproduces the device, whatever the launch shape and the layout.  No operation is fused (no fma); every operation named below rounds
 * once, to nearest even, in IEEE binary32 unless it says double.
 * The set.  S, the box B, lo_k, hi_k and the integer spacing[3] (1 .. VK_DIST_MAX_SPACING) are exactly vk_geodesic_distance's; the box
 * comes from `box`, from the clip box under VK_DIFF_CLIP_BOX, or is the whole volume.  A NaN texel is never in S.  axis a is 0, 1 or 2
 * (x, y, z).  The inlet is B's first index along a, the outlet B's last; a voxel of S is "on the inlet" when its coordinate along a is
 * the inlet's.  n_a is B's extent along a, n_b and n_c its other two.
 * Weights.  w[c] = (float)(1.0 / (double)(spacing[c] * spacing[c])), c = 0, 1, 2 for a neighbour along x, y, z.  g = 2.0f * w[a]: the
 * Dirichlet planes lie half a voxel outside the face voxels' centres.
 * State.  One float c(v) per voxel of S, 0.5f at the start.  Off S there is no value: c_out holds VK_DIFF_OFF there.
 * One voxel's update.  num = den = 0.0f.  For the six neighbours u of v in the order x-, x+, y-, y+, z-, z+, each one that lies in S
 * (a neighbour outside the volume or outside B is not in S): num = num + w * c(u) (the product rounds, then the sum), den = den + w,
 * with w the weight of the neighbour's axis.  If v is on the inlet, num = num + g and den = den + g; if v is on the outlet,
 * den = den + g (a voxel may be on both when n_a == 1).  If den == 0 the voxel is never updated and keeps 0.5f.  Otherwise
 * gs = num / den (correctly rounded), d = gs - c(v), c'(v) = c(v) + omega * d (the product rounds, then the sum).
 * Sweep.  A sweep updates all voxels of S with ((x + y + z) & 1) == 0, on absolute volume indices, then all those with parity 1.  A
 * voxel of one parity has neighbours of the other parity only, so the result of a sweep depends on no order.
 * omega.  req->omega in (0, 2), or 0 for the automatic one: (float)(2.0 / (1.0 + 3.141592653589793 / (double)(n_a + 1))), plain double
 * arithmetic, or the largest float below 2 where the conversion rounds to 2 (n_a above 10^8).  result->omega is the value used.
 * Stopping.  Sweeps run in blocks of check_every (1 .. VK_DIFF_MAX_CHECK_EVERY); at most max_sweeps / check_every blocks run
 * (max_sweeps >= check_every).  After a block:
 *   delta   the largest fabsf(c'(v) - c(v)) (the difference rounds) over the voxels updated in the block's last sweep, 0 if none;
 *   Fin_q   the sum of q(2.0f * (1.0f - c(v))) over the voxels of S on the inlet;
 *   Fout_q  the sum of q(2.0f * c(v)) over the voxels of S on the outlet;
 *   q(t) = (int64_t)(clamp(t) * 1073741824.0f), clamp(t) = t >= -1048576.0f ? (t <= 1048576.0f ? t : 1048576.0f) : -1048576.0f (a NaN
 *   gives -1048576.0f); the product is exact, the conversion truncates, the sums are two's-complement 64-bit integers.
 * The call has converged iff, in IEEE double, (double)delta <= (double)delta_tol and
 * fabs((double)Fin_q - (double)Fout_q) <= (double)flux_tol * 0.5 * ((double)Fin_q + (double)Fout_q).  It stops after the first
 * converged block or after the last permitted one.  sweeps = the blocks run * check_every: the number of sweeps run is exactly this
 * rule's, however the implementation batches its launches.  A run that does not converge is VK_OK with converged == 0.
 * result (may be NULL).  n_foreground = |S|; n_inlet, n_outlet = the voxels of S on the two faces; n_box = the voxels of B; sweeps;
 * converged; delta, Fin_q, Fout_q of the last block; sum_c_q = the sum of q(c(v)) over S; omega and gain as used.
 * What derives from the result, in double (the hosts compute these):
 *   flux = ((double)Fin_q + (double)Fout_q) / 2147483648.0       the mean of the two faces' fluxes, in units of D0 * pitch
 *   D_eff / D0 = flux * n_a / (n_b * n_c)                          the pitch cancels out of the ratio; it enters through the solve only
 *   porosity = n_foreground / n_box                               0 for an empty box
 *   tau = porosity / (D_eff / D0)                                 the tortuosity factor; inf when the flux is 0
 *   flux mismatch = |Fin_q - Fout_q| / |0.5 (Fin_q + Fout_q)|     0 when both are 0; inf when they differ and their mean is 0
 *   mean concentration = sum_c_q / (1073741824.0 n_foreground)    0 for an empty set
 * Components of S that touch neither face are a pure-Neumann problem: they stay at 0.5 up to rounding and carry no flux, because
 * flux is measured on the two faces only; they do count in the porosity.  vk_label_components with VK_LABEL_KEEP_SEEDS or
 * KEEP_LARGEST removes them beforehand.  A component that touches one face only settles at that face's concentration.
 * Outputs.  c_out (may be NULL): nx ny nz float, x fastest.  The dense value of a voxel of S is c(v) * gain (gain == 0 asks for 1),
 * off S it is fill_out; both go through vk_label_components' fill rule F.  dense_out (may be NULL) and VK_DIFF_INSTALL behave exactly
 * as vk_geodesic_distance's dense_out and VK_GEO_INSTALL.  Without VK_DIFF_INSTALL no context state changes.  The call blocks, runs
 * on the context's current stream and allocates and frees its own buffers.
 * VK_ERR_INVALID, decided before any launch, outputs untouched ("vk_steady_diffusion: ..."), in this order: a NULL request; lo or hi
 * NaN; lo > hi; an axis above 2; an unknown flag; a spacing of 0 or above VK_DIST_MAX_SPACING; an omega that is not 0 and not inside
 * (0, 2); check_every outside 1 .. VK_DIFF_MAX_CHECK_EVERY; max_sweeps < check_every; a delta_tol or flux_tol that is negative or not
 * finite; a gain or fill_out that is not finite; none of c_out, dense_out, VK_DIFF_INSTALL and result requested; then VK_DIFF_INSTALL
 * while a frame is being recorded; no volume; a box that is inverted or leaves the volume, a box together with VK_DIFF_CLIP_BOX.
 * VK_ERR_UNSUPPORTED ("diffusion: ..."): a BRICKED / QUADS / STAGED or RGBA16F_PAIR volume; a volume of more than 2^32 - 2 voxels.
 * VK_ERR_OOM: a buffer cannot be allocated.  A call that fails later may have written its outputs already; the context's volume is
 * the old one whenever the call does not return VK_OK. */
#define VK_DIFF_OFF 0x7FC00000u
#define VK_DIFF_MAX_CHECK_EVERY 1024
enum { VK_DIFF_CLIP_BOX = 1, VK_DIFF_INSTALL = 2 };
typedef struct vk_diffusion_request {
    float    lo, hi;                       /* the value range, formed exactly as vk_label_components forms lo_k, hi_k */
    uint32_t axis, flags;                  /* 0, 1, 2 for x, y, z; VK_DIFF_CLIP_BOX | VK_DIFF_INSTALL */
    uint32_t spacing[3];                   /* integer voxel pitch per axis x, y, z: 1 .. VK_DIST_MAX_SPACING */
    float    omega;                        /* the over-relaxation factor in (0, 2); 0: automatic */
    uint32_t check_every, max_sweeps;      /* sweeps per block, 1 .. VK_DIFF_MAX_CHECK_EVERY; the most sweeps, >= check_every */
    float    delta_tol, flux_tol;          /* the two stopping bounds: finite, >= 0 */
    float    gain, fill_out;               /* the dense value is c * gain (0: 1); the sample value off S */
} vk_diffusion_request;                    /* 56 bytes */
typedef struct vk_diffusion_result {
    uint64_t n_foreground, n_inlet, n_outlet, n_box;
    int64_t  Fin_q, Fout_q, sum_c_q;
    uint32_t sweeps, converged;
    float    delta, omega, gain;
    uint32_t pad;
} vk_diffusion_result;                     /* 80 bytes */
#ifdef __cplusplus
static_assert(sizeof(vk_diffusion_request) == 56 && sizeof(vk_diffusion_result) == 80, "vk_diffusion_request: 56 bytes, vk_diffusion_result: 80 bytes");
#else
_Static_assert(sizeof(vk_diffusion_request) == 56 && sizeof(vk_diffusion_result) == 80, "vk_diffusion_request: 56 bytes, vk_diffusion_result: 80 bytes");
#endif
int vk_steady_diffusion(vk_ctx *ctx, const vk_diffusion_request *req, const vk_voxel_box *box, float *c_out, void *dense_out,
                        vk_diffusion_result *result);

/* The resample pass: a voxel box of the volume the context holds into a volume of caller-chosen dimensions, by
 * one of three rules, optionally mapped into another scalar format -- crop, resize, make isotropic, window 16-bit data into u8 --
 * without a trip through the host.  Every f32 operation below is rounded once; fmaf is fused where written and nowhere else.
 * Volume and box.  t(x, y, z) is the STORED texel as f32 on the kernel's scale, as in vk_volume_filter (R8 0..255, R16_UNORM 0..65535,
 * R16F the value; PACKED_PAIRS: the u8 value tap + delta).  B is the voxel box, half-open: `box`, the clip box under
 * VK_RESAMPLE_CLIP_BOX (box must then be NULL), or NULL for the whole volume; an empty box is refused.  Per axis nb is B's extent and n
 * the output extent (dims[axis], or nb where that is 0).  Source indices below are relative to B's low corner, and every index is
 * clamped to B, not to the volume: resampling a box equals resampling an upload of that box alone.
 * Geometry.  Output voxel j of an axis covers [j nb / n, (j + 1) nb / n) in box voxels (the voxel-area convention).  All index
 * arithmetic is in 64-bit integers; floor is towards minus infinity; c(i) = min(max(i, 0), nb - 1).
 * VK_RESAMPLE_NEAREST.  The source index per axis is floor((2 j + 1) nb / (2 n)): the voxel that holds the output voxel's centre.
 * Without a value map the stored bits are copied unchanged (labels, masks, NaN payloads).
 * VK_RESAMPLE_LINEAR.  Per axis num = (2 j + 1) nb - n, den = 2 n, i = floor(num / den), r = num - i den,
 * f = (float)((double)r / (double)den); the taps are c(i) and c(i + 1).  lerp(a, b, f) = (f == 0) ? a : fmaf(f, b - a, a) -- an exact
 * hit never meets its neighbour, so an infinite neighbour cannot make it NaN, and the identity resample is exact.  Four lerps along x
 * (with fx, of the tap pairs at (y, z) = (c(iy), c(iz)), (c(iy+1), c(iz)), (c(iy), c(iz+1)), (c(iy+1), c(iz+1))), then two along y
 * with fy (of the first two results, of the last two), then one along z with fz.
 * VK_RESAMPLE_AREA.  Source voxel k of an axis overlaps output voxel j by o = min((j + 1) nb, (k + 1) n) - max(j nb, k n), for
 * k = floor(j nb / n) .. floor(((j + 1) nb - 1) / n) (every such o is > 0), with weight w_k = (float)((double)o / (double)nb).  Three
 * axis reductions in the order x, y, z over unrounded f32 intermediates, as in VK_FILTER_CONVOLVE: acc = w_first * t, then
 * acc = fmaf(w_k, t, acc) in ascending k.  Refused (VK_ERR_UNSUPPORTED) where nb > VK_RESAMPLE_MAX_RATIO * n on some axis: an output
 * voxel has at most VK_RESAMPLE_MAX_RATIO + 1 taps per axis.
 * Value map.  S is the scale of a format: 255 for R8, 65535 for R16_UNORM, 1 for R16F.  The map runs iff the output format differs
 * from the volume's or VK_RESAMPLE_WINDOW is set.  Without the flag lo = 0, hi = 1.  a = S_out / ((hi - lo) S_in) and
 * b = -lo S_out / (hi - lo), both in double from lo and hi as double, each rounded once to f32; v' = fmaf(a, v, b), with v the
 * interpolated value, or under NEAREST the texel as f32.  The window [lo, hi] is in sample values, like a table's domain.
 * Store.  NEAREST without a map copies bits.  Everything else goes through vk_volume_filter's store rule for the output format (the
 * volume's own without a map): R8 and R16_UNORM (uint) rintf(fminf(fmaxf(v, 0), S)), ties to even, a NaN stores 0; R16F f32 -> f16
 * round to nearest even, subnormals kept, overflow to +-inf, any NaN stored as 0x7E00.
 * Output and state.  dense_out (may be NULL): host memory of n_x n_y n_z elements of the output format, x fastest.  result (may be
 * NULL): the output's dimensions and format, the layout installed (0 without VK_RESAMPLE_INSTALL) and the box B.  The call blocks.
 * VK_RESAMPLE_INSTALL behaves exactly as VK_FILTER_INSTALL: the result replaces the context's volume under the table / projection /
 * isosurface / lighting / shadows in force, frames in flight drain, batches are invalidated, the old volume stays on any failure;
 * vk_volume_info then reports the new dimensions, format and layout.  The clip box stays in force in unit-cube coordinates of the
 * NEW volume: after a crop to the clip box, turn it off (vk_set_clip_box(ctx, NULL)) unless the same fractions of the crop are meant.
 * Without VK_RESAMPLE_INSTALL no context state changes.
 * VK_ERR_INVALID, decided before any launch, outputs untouched ("resample: ..."): a NULL request; an unknown mode, flag or format;
 * RGBA16F_PAIR as the output format; an output extent above 65535; under VK_RESAMPLE_WINDOW lo or hi not finite, lo >= hi, or an a or b
 * that is not finite in f32; neither dense_out nor VK_RESAMPLE_INSTALL; an unknown layout; VK_RESAMPLE_INSTALL while a frame is being
 * recorded; a box that is inverted, empty or leaves the volume, a box together with VK_RESAMPLE_CLIP_BOX; no volume.
 * VK_ERR_UNSUPPORTED ("resample: ..."): a BRICKED / QUADS / STAGED or RGBA16F_PAIR source volume; the AREA ratio above
 * VK_RESAMPLE_MAX_RATIO; under VK_RESAMPLE_INSTALL what vk_volume_upload_device refuses for the output: an extent above 8192,
 * PACKED_PAIRS with an output that is not u8, a layout other than LINEAR / PACKED with an R16_UNORM output.  VK_ERR_OOM: a buffer
 * cannot be allocated; the old volume stays. */
enum { VK_RESAMPLE_NEAREST = 0, VK_RESAMPLE_LINEAR = 1, VK_RESAMPLE_AREA = 2 };
enum { VK_RESAMPLE_INSTALL = 1, VK_RESAMPLE_CLIP_BOX = 2, VK_RESAMPLE_WINDOW = 4 };
#define VK_RESAMPLE_KEEP_FORMAT (-1)
#define VK_RESAMPLE_MAX_RATIO 16
typedef struct vk_resample_request {
    int32_t  mode;         /* VK_RESAMPLE_NEAREST / _LINEAR / _AREA */
    uint32_t flags;        /* VK_RESAMPLE_INSTALL | VK_RESAMPLE_CLIP_BOX | VK_RESAMPLE_WINDOW */
    uint32_t dims[3];      /* output extents x, y, z; 0: that axis keeps the box's extent */
    int32_t  format;       /* VK_RESAMPLE_KEEP_FORMAT, VK_FMT_R8_UNORM, VK_FMT_R16_UNORM or VK_FMT_R16_FLOAT */
    int32_t  layout;       /* with INSTALL.  VK_LAYOUT_AUTO: the layout vk_volume_info reports now, or PACKED where that is
                              PACKED_PAIRS and the output is not u8; otherwise any layout vk_volume_upload_device accepts for the
                              output, with its refusals */
    float    lo, hi;       /* with VK_RESAMPLE_WINDOW: the window in sample values */
} vk_resample_request;     /* 36 bytes */
typedef struct vk_resample_result {
    uint32_t dims[3];
    int32_t  format, layout;
    vk_voxel_box box;
} vk_resample_result;      /* 44 bytes */
#ifdef __cplusplus
static_assert(sizeof(vk_resample_request) == 36 && sizeof(vk_resample_result) == 44, "vk_resample_request: 36 bytes, vk_resample_result: 44 bytes");
#else
_Static_assert(sizeof(vk_resample_request) == 36 && sizeof(vk_resample_result) == 44, "vk_resample_request: 36 bytes, vk_resample_result: 44 bytes");
#endif
int vk_volume_resample(vk_ctx *ctx, const vk_resample_request *req, const vk_voxel_box *box, void *dense_out, vk_resample_result *result);
/* What vk_volume_resample would produce for req and box, without launching or writing anything: the output's extents and format (the size
 * of dense_out), the layout an install would land on (0 without VK_RESAMPLE_INSTALL) and the voxel box -- the clip box's voxels under
 * VK_RESAMPLE_CLIP_BOX.  The refusals are vk_volume_resample's, but for "neither dense_out nor VK_RESAMPLE_INSTALL"; a NULL result is
 * VK_ERR_INVALID.  Does not synchronise; changes no state. */
int vk_resample_output(vk_ctx *ctx, const vk_resample_request *req, const vk_voxel_box *box, vk_resample_result *result);

/* GlobalUniformBinding::update, src/context/global_ubo.rs:47-49 (48-byte Uniform, :52-65). */
int vk_set_uniform(vk_ctx *ctx, const void *blob48);
/* CameraBinding::update, src/camera.rs:62-71 (144-byte CameraUniform, :5-11).  Always uploads
 * (the reference's `updated` gate leaves the first frame with an identity camera). */
int vk_set_camera(vk_ctx *ctx, const void *blob144);

/* ---- output surface: HdrBackBuffer::new, src/context/hdr_backbuffer.rs:41-87 ------------- */
/* Every frame slot takes the new shape, cleared.  VK_ERR_OOM ("vk_backbuffer_resize: the backbuffer: ..."): a slot's backbuffer cannot
 * be allocated; the context is then left without a backbuffer in any slot, at 0 x 0 -- vk_render, vk_present and vk_frame_begin refuse
 * with "no backbuffer" -- until a resize succeeds. */
int vk_backbuffer_resize(vk_ctx *ctx, uint32_t width, uint32_t height, int out_format);
int vk_backbuffer_info(vk_ctx *ctx, uint32_t *width, uint32_t *height, int *out_format, void **device_ptr);
/* Clear to the render pass's LoadOp::Clear(BLACK) = (0,0,0,1), examples/bonsai/main.rs:41. */
int vk_backbuffer_clear(vk_ctx *ctx);

/* ---- frames in flight (ABI 5) -------------------------------------------------------------- */
/* The reference records ONE pass per frame and lets its queue run ahead of the GPU: RedrawRequested calls demo.render and
 * Context::render without waiting for the previous frame (src/lib.rs:178-194); Surface::get_current_texture blocks only
 * when every swapchain image is still in use (src/context.rs:252, PresentMode::Fifo at :118).  A frame that is 70 % empty
 * cannot fill the machine on its own, and a caller that learns its camera one frame at a time cannot use vk_render_batch.
 * With k > 1 the context owns a ring of k frame slots -- backbuffer, present targets and step image of their own, each on
 * its own HIP stream -- and the calls between vk_frame_begin and vk_frame_end go to the slot of that frame, so the first
 * waves of frame i + 1 fill the SIMDs that the tail of frame i leaves idle.  k = 1 (the default) is one slot on the
 * context's stream: the behaviour of ABI 4.  Every frame is bitwise the frame the same calls produce with k = 1.
 *
 * Of a ring of three or four, k - 1 frames execute at once and one waits, recorded, in its queue (its stream waits on the GPU for
 * the frame k - 1 before it): the next frame starts the moment one ends, without the host in between.
 *
 * vk_ctx_frames_in_flight: 1 <= k <= VK_MAX_FRAMES_IN_FLIGHT; drains the context, sizes the ring (new slots take the
 *   backbuffer's current shape, cleared) and forgets earlier frame ids.  Refused while a frame is open, and for k > 1 on a
 *   context that runs on a caller's stream (vk_ctx_set_stream).
 * vk_frame_begin (get_current_texture): takes the next slot of the ring, BLOCKING the host until the frame that used it
 *   k frames ago has completed -- at most k frames are ever in flight; with k = 1 the frames follow one another on one
 *   stream and nothing blocks -- and makes it the context's current surface:
 *   vk_render, vk_backbuffer_clear, vk_present, vk_readback, vk_capture_frame, vk_backbuffer_info and the timers address
 *   it.  *frame_id (>= 1, increasing) names the frame.
 * vk_frame_end (queue.submit + frame.present, src/context.rs:294-296): marks the end of the frame's work.
 * vk_frame_wait: blocks until that frame's work has completed (a frame whose slot has been taken again completed long ago).
 * vk_frame_readback / vk_frame_capture: vk_readback / vk_capture_frame of THAT frame, while its slot still holds it
 *   (VK_ERR_INVALID once a later vk_frame_begin has taken the slot); they wait for the frame only, not for the frames
 *   submitted after it.
 * vk_frame_info: the frame's device buffers (backbuffer; Rgba8 present target or NULL) for consumers on the device -- order
 *   them after vk_frame_wait, and finish with them before the vk_frame_begin that reuses the slot k frames later.
 * Outside begin / end the context behaves as before on its current slot.  vk_ctx_sync drains every slot. */
#define VK_MAX_FRAMES_IN_FLIGHT 4
int vk_ctx_frames_in_flight(vk_ctx *ctx, uint32_t k);
int vk_frame_begin(vk_ctx *ctx, uint64_t *frame_id);
int vk_frame_end(vk_ctx *ctx);
int vk_frame_wait(vk_ctx *ctx, uint64_t frame_id);
int vk_frame_readback(vk_ctx *ctx, uint64_t frame_id, void *dst, size_t row_pitch_bytes);
int vk_frame_capture(vk_ctx *ctx, uint64_t frame_id, void *dst, size_t dst_bytes, uint32_t *out_width, uint32_t *out_height,
                     uint32_t *out_padded_bytes_per_row);
int vk_frame_info(vk_ctx *ctx, uint64_t frame_id, void **backbuffer, void **rgba8, int *complete);

/* ---- the hot path ------------------------------------------------------------------------ */
/* One raycast pass over a tile of the backbuffer, asynchronous on the context's stream.
 * NAIVE: RaycastPipeline::record + queue.submit (examples/bonsai/raycast.rs:118-135,
 * examples/bonsai/main.rs:27-57).  COMPUTE: the `single`/`tile` dispatches with their pixel
 * offset (examples/xor/main.rs:223-254, raycast_compute.wgsl:133-144); pixels of the tile that
 * fall outside the backbuffer are dropped like out-of-range textureStores. */
int vk_render(vk_ctx *ctx, int mode, int32_t tile_x, int32_t tile_y, uint32_t tile_w, uint32_t tile_h,
              float dt_scale, uint32_t flags);

/* Multi-GPU partition of one frame: the backbuffer-sized frame is cut into tile_size^2 tiles
 * (row-major; the reference's TILE_SIZE scheme, examples/xor/main.rs:12,77-95); this call
 * renders the tiles at positions q = rank + j*nranks of the heaviest-first order (vk_partition_order)
 * into `compact_out` (device memory, [n_slots][tile_size][tile_size] pixels of the backbuffer's
 * format, slot j <-> position rank + j*nranks; with vk_partition_root_skip the deal is the weighted one).
 * vk_partition_slots gives n_slots (identical on every rank, for a fixed-size gather). */
int vk_partition_slots(uint32_t width, uint32_t height, uint32_t tile_size, uint32_t nranks, uint32_t *n_slots);
/* A lighter share for the root.  Positions are dealt in rounds, one per rank and round; with root_skip = k >= 2 rank 0
 * sits out every k-th round (its share is (k-1)/k of a peer's): rank 0 also receives and un-tiles every frame, and
 * without this the other ranks wait for it.  0 (default): plain round robin.  Set the same value on every rank's
 * context before partitioning; it applies to vk_render_partition, vk_render_batch, vk_untile(_batch) and
 * vk_partition_active.  vk_partition_slots_weighted: the slot count (of a non-root rank) under that deal. */
int vk_partition_root_skip(vk_ctx *ctx, uint32_t root_skip);
int vk_partition_slots_weighted(uint32_t width, uint32_t height, uint32_t tile_size, uint32_t nranks, uint32_t root_skip,
                                uint32_t *n_slots);
/* What a pixel of a partition's compact tiles holds.  VK_WIRE_RGBA (default): the backbuffer's pixel.  VK_WIRE_RGB: its
 * three colour channels -- every pixel this path writes has alpha 1 (raycast_naive.wgsl:124, raycast_compute.wgsl:143),
 * and the tiles exist to be moved over xGMI: 6 bytes instead of 8 per rgba16f pixel, a quarter less on the one link
 * each peer has to the root (which is what bounds an 8-GPU node on the 1080p configuration: DESIGN.md 6).  A (slot,
 * frame) record is then ts*ts (r, g) pairs followed by ts*ts b values; the un-tile writes alpha = 1.  Set the same
 * value on every rank before partitioning; it applies to the compact output of vk_render_partition / vk_render_batch,
 * to vk_gather_tiles (n_pixels counts pixels of this size) and to vk_untile / vk_untile_batch.  Frames are bitwise
 * what VK_WIRE_RGBA delivers.  vk_wire_pixel_bytes: bytes per pixel of the context's compact tiles. */
enum { VK_WIRE_RGBA = 0, VK_WIRE_RGB = 1 };
int vk_partition_wire(vk_ctx *ctx, int wire);
int vk_wire_pixel_bytes(vk_ctx *ctx, uint32_t *bytes);
/* The tiles a partition marches and moves ("active"): those the box's projected silhouette -- the convex hull of its 8
 * corners under this camera, 2 px of margin -- can reach; every other tile holds only the clear colour
 * (examples/bonsai/main.rs:41) and is cleared by the root.  Pure host arithmetic, no context: active[] receives
 * tiles_x * tiles_y bytes (row-major, 1 = active).  vk_partition_active reports the same count for a context's camera. */
int vk_tiles_active(const void *camera144, int mode, uint32_t width, uint32_t height, uint32_t tile_size,
                    unsigned char *active, uint32_t *n_active);
int vk_render_partition(vk_ctx *ctx, int mode, uint32_t tile_size, uint32_t rank, uint32_t nranks,
                        float dt_scale, uint32_t flags, void *compact_out);
/* The partition deals tiles heaviest-first (a launch/balance heuristic derived from the camera):
 * position q of the order belongs to rank q % nranks, slot q / nranks.  order_out[q] = row-major
 * tile id; identical on every rank for identical camera, volume dims and backbuffer size. */
int vk_partition_order(vk_ctx *ctx, int mode, uint32_t tile_size, uint32_t *order_out, uint32_t n_tiles);
/* Only the leading n_active_tiles positions of the order can hold non-clear pixels (tiles touching the
 * cube's screen rectangle); vk_render_partition marches just those, so a rank's compact buffer is
 * meaningful in its first n_active_slots = ceil(n_active_tiles / nranks) slots and only those need
 * to be gathered.  Camera-dependent; identical on every rank. */
int vk_partition_active(vk_ctx *ctx, int mode, uint32_t tile_size, uint32_t nranks, uint32_t *n_active_tiles,
                        uint32_t *n_active_slots);
/* Root side: scatter the gathered [nranks][slot_stride][ts][ts] pixels into the backbuffer; tiles beyond
 * the active ones are cleared to (0,0,0,1).  Uses the order of the LAST partition call on this context, so
 * frames marched before a camera change are un-tiled as they were dealt: deliver them before the next
 * partition call under the new camera.  (A stream of frames with changing cameras: vk_render_batch.) */
int vk_untile(vk_ctx *ctx, const void *gathered, uint32_t tile_size, uint32_t nranks, uint32_t slot_stride);
/* Several frames in ONE launch.  The reference keeps frames in flight through its queue (src/lib.rs:178-194 submits a
 * frame per RedrawRequested without waiting); here the grid itself spans n_frames frames, each with its own camera
 * (`cameras`: n_frames x 144-byte CameraUniform blobs, host memory) and its own heaviest-first tile order, dealt
 * position-major so the heaviest tiles of every frame start first.  A frame that is 70 % empty cannot fill 8192 wave
 * slots on its own; a batch can, and a rank holding 1/N of every frame still has n_frames/N frames of work per launch.
 *   compact == 0: `out` receives whole frames (nranks == 1; a rank's share of them with nranks > 1, see below), [n_frames][height][width] pixels of the
 *     backbuffer's format.
 *   compact != 0: `out` receives this rank's tiles, [slot][frame][ts][ts] (slot j <-> position rank + j*nranks of
 *     that frame's order), slot < *n_active_slots <= slot_capacity: a contiguous prefix, ready for one gather.
 * n_frames <= VK_MAX_BATCH_FRAMES.  *batch_id names the batch's tables for vk_untile_batch (the library holds the last 4; a
 * vk_backbuffer_resize or a new volume drops them all).  VK_RENDER_COUNT is refused.
 * Every frame is bitwise equal to the one vk_render produces for the same camera. */
#define VK_MAX_BATCH_FRAMES 1024
/* compact == 0 with nranks > 1 (ABI 4): this rank's tiles written at their place in whole frames [n_frames][height][width] that `out` addresses --
 * typically another GPU's memory, mapped by hipDeviceEnablePeerAccess (vk_group_peer_direct) or HIP IPC: peer-direct tiles, no gather and no
 * un-tile.  Rank 0 also clears the tiles the silhouette cannot reach.  The caller orders the ranks' launches against the consumer. */
int vk_render_batch(vk_ctx *ctx, int mode, uint32_t n_frames, const void *cameras, uint32_t tile_size, uint32_t rank,
                    uint32_t nranks, float dt_scale, uint32_t flags, void *out, int compact, uint32_t slot_capacity,
                    uint32_t *batch_id, uint32_t *n_active_slots);
/* Root side of a batch: gathered [nranks][n_slots][frame][ts][ts] -> out_frames [n_frames][height][width].
 * A batch in which no frame has an active tile (*n_active_slots == 0) still has every frame cleared by this call, and `gathered` is
 * still checked: NULL is VK_ERR_INVALID even though nothing is read through it -- pass any device pointer with n_slots = 0. */
int vk_untile_batch(vk_ctx *ctx, uint32_t batch_id, const void *gathered, uint32_t n_slots, void *out_frames);
/* The same when out_frames still holds, untouched, what un-tiling `prev_batch_id` (one of the last 4 batches, same frame count
 * and shape) wrote there -- a driver that alternates two frame buffers passes the batch before last: tiles that were inactive
 * then and are inactive now keep their clear colour and are not written again (most of a frame under a still or slowly moving
 * camera: 10.5 of the 22.8 MB an un-tile moves per C2 frame).  prev_batch_id = 0, or a batch that no longer fits: a full
 * un-tile. */
int vk_untile_batch_over(vk_ctx *ctx, uint32_t batch_id, const void *gathered, uint32_t n_slots, void *out_frames, uint32_t prev_batch_id);

/* ---- multi-GPU: the framebuffer's tiles over the node's GPUs, RCCL over xGMI ------------- */
/* Generalises the reference's tile loop (examples/xor/main.rs:235-254: one dispatch per 256x256 tile) to one GPU per
 * share of the tiles.  The volume is replicated (upload it on every context); there is no reduction, only the
 * gather of finished tiles to the root.  RCCL is loaded on first use.
 *
 * (a) one process per GPU (MPI / torchrun style): rank 0 makes an id, the host ships its 128 bytes to the peers,
 *     every rank joins; then per batch vk_render_batch(compact) -> vk_gather_tiles -> (root) vk_untile_batch. */
#define VK_COMM_ID_BYTES 128
/* Can this process load and bind RCCL (librccl.so.1, or what VK_RCCL_LIB names)?  VK_OK, or VK_ERR_UNSUPPORTED with the reason in
 * vk_last_error(NULL).  No side effect beyond loading the library: the probe every rank can make before any of them enters the
 * blocking vk_comm_init_rank.  (vk_comm_unique_id opens a bootstrap listener for the ranks to come: call it on ONE rank.) */
int vk_comm_available(void);
int vk_comm_unique_id(void *id128);
int vk_comm_init_rank(vk_ctx *ctx, const void *id128, int rank, int nranks);
int vk_comm_destroy(vk_ctx *ctx);
/* ABI 5.  Tear the communicator down WITHOUT waiting for what is in flight (ncclCommAbort): for a rank that has found a peer gone -- a
 * gather that does not complete within the caller's time limit (vk_comm_destroy would wait on the stream the dead transfer sits on).
 * Transfers in flight are cancelled, the buffers they were writing are undefined; the context stays usable and may join a new
 * communicator.  No-op without a communicator. */
int vk_comm_abort(vk_ctx *ctx);
int vk_comm_info(vk_ctx *ctx, int *rank, int *nranks);
/* Every rank contributes n_pixels pixels (of the partition's wire format: vk_partition_wire) from `send`; the root receives [nranks][n_pixels] in
 * `recv` (ignored elsewhere).  One grouped send/recv, asynchronous, on `hip_stream` (NULL: the context's stream; a
 * separate stream lets the gather of one batch overlap the march of the next -- the caller orders the two). */
int vk_gather_tiles(vk_ctx *ctx, const void *send, void *recv, size_t n_pixels, int root, void *hip_stream);
/* (b) one process for the node: a group owns one context per GPU (ncclCommInitAll).  Upload the volume and size the
 *     backbuffer on every member (vk_group_ctx), then vk_group_render marches, gathers and un-tiles n_frames frames
 *     into out_frames ([n_frames][height][width], device memory of GPU ordinals[0]).  Asynchronous; vk_group_sync
 *     waits for every member. */
typedef struct vk_group vk_group;
int vk_group_create(int n, const int *ordinals, vk_group **out);
int vk_group_destroy(vk_group *g);
int vk_group_size(vk_group *g);
vk_ctx *vk_group_ctx(vk_group *g, int i);
int vk_group_render(vk_group *g, int mode, uint32_t n_frames, const void *cameras, uint32_t tile_size, float dt_scale,
                    uint32_t flags, void *out_frames);
/* Peer-direct tiles (enable != 0): every member's march stores its pixels straight into out_frames on GPU ordinals[0] over xGMI
 * (hipDeviceEnablePeerAccess) -- no staging buffer, no gather, no un-tile pass on the root, whose fixed 5 us per 1080p frame is what
 * bounds the gathered path at 8 GPUs.  The price: the stores cross the link as they are issued, 8 bytes at a time per lane, instead of
 * in one bulk transfer.  Frames are bitwise the same.  Fails (and leaves the gathered path in place) when a member cannot access
 * the root's memory.  The members write out_frames from their OWN streams (the root's stream waits for them, not they for it): a second
 * vk_group_render into the same out_frames must not be issued before whatever reads the first one's frames on the root has finished
 * (vk_group_sync, or alternate two buffers). */
int vk_group_peer_direct(vk_group *g, int enable);
int vk_group_sync(vk_group *g);
const char *vk_group_last_error(vk_group *g);

/* Device memory for hosts that have no other allocator (frame batches, gather buffers).  vk_device_free and
 * vk_device_download synchronise the context's stream. */
int vk_device_alloc(vk_ctx *ctx, size_t bytes, void **ptr);
int vk_device_free(vk_ctx *ctx, void *ptr);
int vk_device_download(vk_ctx *ctx, void *dst_host, const void *src_device, size_t bytes);

/* ---- present + screenshot ---------------------------------------- */
/* Context::render's present pass (src/context.rs:251-297, shaders/present.wgsl:23-35,111-119): bilinear
 * resample of the backbuffer to width x height (the window size), ACESFilm, linear_to_srgb, into the
 * context-owned Rgba8Unorm target (and a Bgra8Unorm "surface" copy when also_bgra != 0).  Asynchronous. */
/* What it computes, per pixel (x, y) of the window and per channel (tests/np_present_reference.py restates this in float64):
 *   - the sample position and weights are this f32 chain: uv = (x + 0.5) / width, u = fma(uv, backbuffer_width, -0.5), texel floor(u) and
 *     floor(u) + 1 clamped to the edge, weight fract(u) (below 1); the same in y.  They are part of the specification.
 *   - a sample whose two weights are both exactly 0 is that texel's value, whatever its neighbours hold; otherwise the bilinear blend
 *     a + fx (b - a) follows IEEE: a NaN tap, or inf - inf, makes NaN.
 *   - colour = linear_to_srgb(ACESFilm(v)) as real functions of present.wgsl:23-35 (exponent 0.41666, threshold 0.0031308), ACESFilm extended
 *     by its limits: huge finite values and +-inf map to 1.  Alpha is v itself.  NaN maps to 0 in every channel, alpha included.
 *   - clamp to [0, 1], times 255, round half up.  Bgra8 is Rgba8 with bytes 0 and 2 exchanged. */
int vk_present(vk_ctx *ctx, uint32_t width, uint32_t height, int also_bgra);
/* The current frame slot's present targets, device pointers to width x height tightly packed 4-byte pixels: the Rgba8Unorm image
 * vk_capture_frame reads and the Bgra8Unorm surface copy (NULL when no present has asked for one at this size; it holds the last present
 * that did).  Every out-pointer is optional.  VK_ERR_INVALID before anything was presented.  Does not synchronise: order reads after the
 * context's stream (vk_ctx_sync, vk_device_download). */
int vk_present_info(vk_ctx *ctx, uint32_t *width, uint32_t *height, void **rgba8, void **bgra8);
/* Context::capture_frame (src/context.rs:299-302, src/context/screenshot.rs:37-77): the presented Rgba8
 * image with the reference's ImageDimentions: even-rounded size, rows padded to 256 B.  dst == NULL only
 * queries the three sizes.  Blocking. */
int vk_capture_frame(vk_ctx *ctx, void *dst, size_t dst_bytes, uint32_t *out_width, uint32_t *out_height,
                     uint32_t *out_padded_bytes_per_row);

/* ---- results ----------------------------------------------------------------------------- */
/* ScreenshotCtx::capture_frame's copy_texture_to_buffer + map, src/context/screenshot.rs:37-77.
 * Blocking.  row_pitch_bytes >= width * bytes_per_pixel. */
int vk_readback(vk_ctx *ctx, void *dst, size_t row_pitch_bytes);
/* Counters of the launches since the last reset (flag VK_RENDER_COUNT): loop iterations the
 * reference would execute (S_ref) and iterations in which taps were fetched (S_sampled). */
int vk_step_counts(vk_ctx *ctx, uint64_t *s_ref, uint64_t *s_sampled);
int vk_step_counts_reset(vk_ctx *ctx);
/* SIMT execution census of the VK_RENDER_COUNT launches since the last reset (NAIVE mode):
 * out[0] wave-level march-loop iterations, out[1] wave-level skipped-step iterations,
 * out[2] wave-level sample executions, out[3] per-lane march-loop iterations (lookups). */
int vk_simt_census(vk_ctx *ctx, uint64_t out[4]);
/* Lone-speckle census of the built-in skip kernels, same launches: out[0] wave-level sample executions in which every sampling
 * lane's alpha was 0 (the palette and the compositing were left out), out[1] lane-steps that a cell's speckle code proved
 * transparent without a sample (they count in S_ref and in S_sampled like the samples they replace). */
int vk_speckle_census(vk_ctx *ctx, uint64_t out[2]);
/* Debug: override the tile order table of the last launch's partition (experiments on launch order): `order` is a permutation of
 * the n tiles (position -> row-major tile id) that keeps the active tiles -- the leading vk_partition_active positions of the
 * current order, the only ones a launch marches -- in front; anything else is VK_ERR_INVALID.  It stays until the partition's
 * key (camera, volume, tile size, rectangle) changes.  The frame does not depend on the order. */
int vk_debug_set_tile_order(vk_ctx *ctx, const uint32_t *order, uint32_t n);
/* Debug: the skip maps of the current volume as the marches read them; read-only.  grid: the stored grid in cells per axis (4 per
 * brick, padding bricks included); n_maps: 0 for a layout without maps (LINEAR, BRICKED, QUADS, STAGED), 1 for the isotropic map, 8 for
 * the one-sided octant maps (octant o = ux | uy << 1 | uz << 2, bit set: the rays go up that axis); bytes: n_maps * cells.  dst == NULL
 * only queries the three; otherwise the frame slots are drained and the maps are copied out as stored: one byte per cell, cell
 * (x, y, z) of brick (x >> 2, y >> 2, z >> 2) at 64 * ((bz * nby + by) * nbx + bx) + (z & 3) << 4 | (y & 3) << 2 | (x & 3), octant o at
 * o * cells.  A PACKED RGBA16F_PAIR volume reports one map over its record grid, each byte taken out of its record.  NULL grid,
 * n_maps or bytes, dst_bytes < bytes, or no volume uploaded: VK_ERR_INVALID.  Blocking. */
int vk_debug_read_skip_maps(vk_ctx *ctx, uint32_t grid[3], uint32_t *n_maps, size_t *bytes, void *dst, size_t dst_bytes);
/* Debug: per-8x8-block {first start, last end, HW_ID | XCC_ID << 32, work} of the next VK_RENDER_COUNT NAIVE
 * launch (s_memrealtime stamps).  enable != 0 arms it; out != NULL copies n_blocks quadruples back. */
int vk_debug_wave_trace(vk_ctx *ctx, int enable, uint64_t *out, size_t n_blocks);
/* Debug / tuning knobs of the staged march: "stage_cap_bytes" (LDS window per wave; 0 = default: 8192 for u8, 10240 for f16),
 * "stage_slab_cells" (a round is a slab of at most that many cells along the wave's major axis, default 8), "stage_copies_mask" (bit k: build the brick copy
 * whose slow axis is k; applies to the next upload, default 7).
 * Tests: "alloc_fail_at" k -- the k-th device or pinned-host allocation the library makes for this context from now on (k >= 1) fails as
 * an allocation that does not fit fails (VK_ERR_OOM with the call's own message), once: the parameter then disarms itself.  0 disarms;
 * setting it again restarts the count.  The allocation asks the runtime for 2^60 bytes in place of its size, so nothing is exhausted.
 * What a failed call leaves behind is the documented contract of each entry point. */
int vk_debug_set_param(vk_ctx *ctx, const char *name, double value);
/* Debug: which build of the cell march vk_render(ctx, VK_MODE_NAIVE_TRILINEAR, ..., dt_scale, flags) would launch now, for the context's
 * volume and camera: *fast = 1 the unclamped build (index tables in LDS, 32-bit offsets), 0 the clamped one (VK_RENDER_SAFE's).  The
 * answer of the function the launch itself asks (the cell array under 4 GiB, the tables within their LDS budget, and camera distance and
 * ray length -- max(dims) / dt_scale trips -- small enough that f32 drift keeps every index inside the tables); 0 on the layouts that are
 * always clamped (LINEAR, BRICKED, QUADS, STAGED).  Frames are the same bits on either build.  No volume, no camera, fast == NULL or a
 * dt_scale that is not finite and > 0: VK_ERR_INVALID.  Host code only. */
int vk_debug_march_path(vk_ctx *ctx, float dt_scale, uint32_t flags, int *fast);
/* Per-pixel executed loop iterations of the last VK_RENDER_COUNT launch ([height][width] u32). */
int vk_readback_steps(vk_ctx *ctx, uint32_t *dst);

/* hipEvent bracket on the context's stream -- the analogue of the reference's timestamp
 * queries around the raycast pass (examples/xor/main.rs:217,258-259,164-187). */
int vk_timer_begin(vk_ctx *ctx);
int vk_timer_end(vk_ctx *ctx);
int vk_timer_elapsed_ms(vk_ctx *ctx, float *ms); /* blocks until the end event has passed */

/* dispatch_optimal, src/utils/mod.rs:15-18 */
uint32_t vk_dispatch_optimal(uint32_t len, uint32_t subgroup_size);

#ifdef __cplusplus
}
#endif
#endif /* VOKSELIS_HIP_H */
