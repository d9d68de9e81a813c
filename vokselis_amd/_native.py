"""ctypes binding of the C-ABI in include/vokselis_hip.h (libvokselis_hip.so).

There is no CPU fallback: if the shared library is missing, or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libvokselis_hip.so")

VK_OK = 0
FMT_R8_UNORM, FMT_R16_FLOAT, FMT_RGBA16F_PAIR, FMT_R16_UNORM = 0, 1, 2, 3
MODE_NAIVE_TRILINEAR, MODE_COMPUTE_NEAREST, MODE_PROCEDURAL = 0, 1, 2
OUT_RGBA32F, OUT_RGBA16F = 0, 1
LAYOUT_AUTO, LAYOUT_LINEAR, LAYOUT_PACKED, LAYOUT_PACKED_PAIRS, LAYOUT_BRICKED, LAYOUT_QUADS, LAYOUT_STAGED = 0, 1, 2, 3, 4, 5, 6
RENDER_NO_SKIP, RENDER_COUNT, RENDER_SAFE, RENDER_FORCE_SKIP = 1, 2, 4, 8
RENDER_DEBUG_TRIPS = 16
RENDER_DEBUG_FALLBACK, RENDER_PROBE_ALWAYS, RENDER_FAST_WALK = 32, 64, 128
RENDER_PRESENT, RENDER_PRESENT_BGRA, RENDER_PRESENT_ONLY = 256, 512, 1024
RENDER_DEVICE_SINE = 2048
WIRE_RGBA, WIRE_RGB = 0, 1
MAX_FRAMES_IN_FLIGHT = 4
GEN_FOG, GEN_BONSAI_STANDIN, GEN_FOG_DENSE_CORE = 0, 1, 2
TF_MAX_ENTRIES = 256
PROJ_COMPOSITE, PROJ_MAX = 0, 1
ISO_MAX_REFINE = 16


class VkLighting(C.Structure):
    """vk_lighting (32 bytes): the light's direction (towards the light), headlight, and the Blinn-Phong coefficients."""
    _fields_ = [("dir", C.c_float * 3), ("headlight", C.c_int32), ("ambient", C.c_float), ("diffuse", C.c_float),
                ("specular", C.c_float), ("shininess", C.c_float)]


assert C.sizeof(VkLighting) == 32


class VkIsosurface(C.Structure):
    """vk_isosurface (20 bytes): the threshold in sample values, the linear surface colour, the bisection steps at the hit."""
    _fields_ = [("iso", C.c_float), ("rgb", C.c_float * 3), ("refine", C.c_uint32)]


assert C.sizeof(VkIsosurface) == 20


class VkShadows(C.Structure):
    """vk_shadows (8 bytes): how much of the diffuse and specular terms a shadowed point loses, and the first shadow sample's distance."""
    _fields_ = [("strength", C.c_float), ("bias", C.c_float)]


assert C.sizeof(VkShadows) == 8

class VkClipBox(C.Structure):
    """vk_clip_box (24 bytes): the clip box of the table, lit, MAX and isosurface marches, lo and hi per axis in unit-cube coordinates."""
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3)]


assert C.sizeof(VkClipBox) == 24


class VkHit(C.Structure):
    """vk_hit (36 bytes): one pixel's record of the geometry pass (vk_pick) -- hit, the crossing, its distance along the ray, the raw
    gradient and the sample value there."""
    _fields_ = [("hit", C.c_int32), ("pos", C.c_float * 3), ("t", C.c_float), ("grad", C.c_float * 3), ("value", C.c_float)]


assert C.sizeof(VkHit) == 36
GEOM_RECORD_BYTES = 32  # a pixel of the geometry surface: two float4

SLAB_MAX, SLAB_MIN, SLAB_MEAN = 0, 1, 2
SLICE_VALUES = 1
SLICE_MAX_SAMPLES = 256
SLICE_MAX_COORD = 1e6
SLICE_RECORD_BYTES = 8  # a pixel of the slice pass's value surface: (x, weight) f32


class VkSlice(C.Structure):
    """vk_slice (56 bytes): the plane of a slice pass in unit-cube coordinates -- the position of the centre of backbuffer pixel (0, 0), the
    change per pixel in +x and +y, the change per slab sample -- and the slab: its samples and their reduction."""
    _fields_ = [("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("dn", C.c_float * 3), ("samples", C.c_uint32),
                ("reduce", C.c_int32)]


assert C.sizeof(VkSlice) == 56


class VkSliceSample(C.Structure):
    """vk_slice_sample (20 bytes): one pixel of a slice (vk_slice_probe) -- whether its position lies in the box, the position, the value."""
    _fields_ = [("inside", C.c_int32), ("pos", C.c_float * 3), ("value", C.c_float)]


assert C.sizeof(VkSliceSample) == 20


HIST_MAX_BINS = 4096
HIST_CLIP_BOX = 1


class VkHistogram(C.Structure):
    """vk_histogram (16 bytes): the request of vk_volume_histogram -- the domain in sample values, the bins, the flags."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("bins", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(VkHistogram) == 16


class VkVoxelBox(C.Structure):
    """vk_voxel_box (24 bytes): the voxels [x0, x1) x [y0, y1) x [z0, z1)."""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("z0", C.c_uint32), ("x1", C.c_uint32), ("y1", C.c_uint32), ("z1", C.c_uint32)]


assert C.sizeof(VkVoxelBox) == 24


class VkVolumeStats(C.Structure):
    """vk_volume_stats (72 bytes): the categories, the f64 sums over the finite texels, min and max -- all on the kernel's scale -- and that scale."""
    _fields_ = [("n_voxels", C.c_uint64), ("n_nan", C.c_uint64), ("n_below", C.c_uint64), ("n_above", C.c_uint64), ("n_finite", C.c_uint64),
                ("sum", C.c_double), ("sum_sq", C.c_double), ("min", C.c_float), ("max", C.c_float), ("scale", C.c_float), ("pad", C.c_uint32)]


assert C.sizeof(VkVolumeStats) == 72


MESH_CLIP_BOX = 1


class VkMeshRequest(C.Structure):
    """vk_mesh_request (8 bytes): the request of vk_extract_isosurface -- the threshold in sample values, the flags."""
    _fields_ = [("iso", C.c_float), ("flags", C.c_uint32)]


assert C.sizeof(VkMeshRequest) == 8


FILTER_MAX_RADIUS = 6
FILTER_MAX_WEIGHT = 1024.0
FILTER_CONVOLVE, FILTER_MEDIAN3 = 0, 1
FILTER_INSTALL = 1


class VkVolumeFilter(C.Structure):
    """struct vk_volume_filter (176 bytes): the request of vk_volume_filter -- the op, the flags, the radius per axis (x, y, z) and the
    2 r + 1 weights of each axis."""
    _fields_ = [("op", C.c_int32), ("flags", C.c_uint32), ("radius", C.c_uint32 * 3), ("weights", (C.c_float * (2 * FILTER_MAX_RADIUS + 1)) * 3)]


assert C.sizeof(VkVolumeFilter) == 176


LABEL_MAX_SEEDS = 16
LABEL_KEEP_ALL, LABEL_KEEP_LARGEST, LABEL_KEEP_MIN_SIZE, LABEL_KEEP_SEEDS = 0, 1, 2, 3
LABEL_CLIP_BOX, LABEL_INSTALL, LABEL_INVERT = 1, 2, 4


class VkLabelRequest(C.Structure):
    """vk_label_request (232 bytes): the request of vk_label_components -- the value range, the connectivity, the flags, what to keep
    (with its count or its seeds) and the fill."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("connectivity", C.c_uint32), ("flags", C.c_uint32), ("keep", C.c_int32), ("n_seeds", C.c_uint32),
                ("count", C.c_uint64), ("fill", C.c_float), ("pad", C.c_uint32), ("seeds", (C.c_uint32 * 3) * LABEL_MAX_SEEDS)]


class VkComponent(C.Structure):
    """vk_component (40 bytes): a component's voxels, its smallest linear index and its tight half-open bounding box."""
    _fields_ = [("n_voxels", C.c_uint64), ("first", C.c_uint64), ("box", VkVoxelBox)]


class VkLabelResult(C.Structure):
    """vk_label_result (32 bytes): the totals of vk_label_components."""
    _fields_ = [("n_components", C.c_uint64), ("n_foreground", C.c_uint64), ("n_kept_components", C.c_uint64), ("n_kept_voxels", C.c_uint64)]


assert C.sizeof(VkLabelRequest) == 232 and C.sizeof(VkComponent) == 40 and C.sizeof(VkLabelResult) == 32


DIST_INF = 0xFFFFFFFF
DIST_MAX_SPACING = 64
DIST_MAX_RADIUS = 65535.0
DIST_OUTSIDE, DIST_INSIDE, DIST_DILATE, DIST_ERODE, DIST_CLOSE, DIST_OPEN = 0, 1, 2, 3, 4, 5
DIST_CLIP_BOX, DIST_INSTALL = 1, 2


class VkDistanceRequest(C.Structure):
    """vk_distance_request (40 bytes): the request of vk_distance_transform -- the value range, the op, the flags, the integer spacing
    per axis (x, y, z), the radius of a morphology op and the two fills."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("op", C.c_int32), ("flags", C.c_uint32), ("spacing", C.c_uint32 * 3), ("radius", C.c_float),
                ("fill_in", C.c_float), ("fill_out", C.c_float)]


class VkDistanceResult(C.Structure):
    """vk_distance_result (40 bytes): the counts of vk_distance_transform, and the largest finite squared distance of a distance op."""
    _fields_ = [("n_foreground", C.c_uint64), ("n_result", C.c_uint64), ("n_added", C.c_uint64), ("n_removed", C.c_uint64), ("max_d2", C.c_uint32), ("pad", C.c_uint32)]


assert C.sizeof(VkDistanceRequest) == 40 and C.sizeof(VkDistanceResult) == 40


SPLIT_CLIP_BOX, SPLIT_INSTALL = 1, 2


class VkSplitRequest(C.Structure):
    """vk_split_request (40 bytes): the request of vk_split_components -- the value range, the connectivity, the flags, the integer
    spacing per axis (x, y, z), the erosion radius and the fill of a cut voxel."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("connectivity", C.c_uint32), ("flags", C.c_uint32), ("spacing", C.c_uint32 * 3), ("radius", C.c_float),
                ("fill_out", C.c_float), ("pad", C.c_uint32)]


class VkSplitResult(C.Structure):
    """vk_split_result (64 bytes): the totals of vk_split_components."""
    _fields_ = [("n_regions", C.c_uint64), ("n_foreground", C.c_uint64), ("n_markers", C.c_uint64), ("n_marker_voxels", C.c_uint64), ("n_residue_regions", C.c_uint64),
                ("n_residue_voxels", C.c_uint64), ("n_cut", C.c_uint64), ("rounds", C.c_uint32), ("pad", C.c_uint32)]


assert C.sizeof(VkSplitRequest) == 40 and C.sizeof(VkSplitResult) == 64


MEASURE_CLIP_BOX = 1


class VkMeasureRequest(C.Structure):
    """vk_measure_request (24 bytes): the request of vk_measure_components -- the value range, the connectivity and the flags where the
    library labels the regions itself; max_label where the caller brings the labels (everything else is 0 then)."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("connectivity", C.c_uint32), ("flags", C.c_uint32), ("max_label", C.c_uint32), ("pad", C.c_uint32)]


class VkRegion(C.Structure):
    """vk_region (192 bytes): a region's exact integer record -- voxels, first voxel, box, the sums of the voxel indices and of their
    products, the texel's extremes and 128-bit sums on the integer scale q, the exposed faces per axis."""
    _fields_ = [("n_voxels", C.c_uint64), ("first", C.c_uint64), ("box", VkVoxelBox), ("sum_x", C.c_uint64), ("sum_y", C.c_uint64), ("sum_z", C.c_uint64),
                ("sum_xx", C.c_uint64), ("sum_yy", C.c_uint64), ("sum_zz", C.c_uint64), ("sum_xy", C.c_uint64), ("sum_xz", C.c_uint64), ("sum_yz", C.c_uint64),
                ("n_nonfinite", C.c_uint64), ("q_min", C.c_int64), ("q_max", C.c_int64), ("sum_q_hi", C.c_int64), ("sum_q_lo", C.c_uint64),
                ("sum_qq_hi", C.c_uint64), ("sum_qq_lo", C.c_uint64), ("faces", C.c_uint64 * 3)]


class VkMeasureResult(C.Structure):
    """vk_measure_result (32 bytes): the totals of vk_measure_components and the divisor from q to the sample value."""
    _fields_ = [("n_regions", C.c_uint64), ("n_foreground", C.c_uint64), ("records_written", C.c_uint64), ("scale", C.c_uint32), ("pad", C.c_uint32)]


assert C.sizeof(VkMeasureRequest) == 24 and C.sizeof(VkRegion) == 192 and C.sizeof(VkMeasureResult) == 32


THICK_MAX_REACH = 32
THICK_CLIP_BOX, THICK_INSTALL = 1, 2


class VkThicknessRequest(C.Structure):
    """vk_thickness_request (36 bytes): the request of vk_local_thickness -- the value range, the flags, the integer spacing per axis
    (x, y, z), the cap of the radius, the gain of the dense value (0: automatic) and the fill of a voxel outside the set."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("flags", C.c_uint32), ("spacing", C.c_uint32 * 3), ("max_radius", C.c_float), ("gain", C.c_float),
                ("fill_out", C.c_float)]


class VkThicknessResult(C.Structure):
    """vk_thickness_result (32 bytes): the totals of vk_local_thickness and the gain it used."""
    _fields_ = [("n_foreground", C.c_uint64), ("n_saturated", C.c_uint64), ("sum_t2", C.c_uint64), ("max_t2", C.c_uint32), ("gain", C.c_float)]


assert C.sizeof(VkThicknessRequest) == 36 and C.sizeof(VkThicknessResult) == 32


GEO_INF, GEO_FAR, GEO_UNIT, GEO_MAX_SEEDS = 0xFFFFFFFF, 0xFFFFFFFE, 256, 16
GEO_CLIP_BOX, GEO_INSTALL = 1, 2
GEO_FACE_X0, GEO_FACE_X1, GEO_FACE_Y0, GEO_FACE_Y1, GEO_FACE_Z0, GEO_FACE_Z1 = 1, 2, 4, 8, 16, 32


class VkGeodesicRequest(C.Structure):
    """vk_geodesic_request (248 bytes): the request of vk_geodesic_distance -- the value range, the connectivity, the flags, the integer
    spacing per axis (x, y, z), the source and target face masks, the seeds in use, the gain of the dense value (0: automatic), the fills
    of a voxel outside the set and of an unreached voxel of it, and the seeds as voxel indices (x, y, z)."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("connectivity", C.c_uint32), ("flags", C.c_uint32), ("spacing", C.c_uint32 * 3), ("source_faces", C.c_uint32),
                ("target_faces", C.c_uint32), ("n_seeds", C.c_uint32), ("gain", C.c_float), ("fill_out", C.c_float), ("fill_unreached", C.c_float), ("pad", C.c_uint32),
                ("seeds", (C.c_uint32 * 3) * GEO_MAX_SEEDS)]


class VkGeodesicResult(C.Structure):
    """vk_geodesic_result (64 bytes): the totals of vk_geodesic_distance and the gain it used."""
    _fields_ = [("n_foreground", C.c_uint64), ("n_sources", C.c_uint64), ("n_reached", C.c_uint64), ("n_saturated", C.c_uint64), ("n_target_reached", C.c_uint64),
                ("sum_g", C.c_uint64), ("max_g", C.c_uint32), ("target_min", C.c_uint32), ("gain", C.c_float), ("pad", C.c_uint32)]


assert C.sizeof(VkGeodesicRequest) == 248 and C.sizeof(VkGeodesicResult) == 64


SKEL_CURVE, SKEL_KERNEL = 0, 1
SKEL_CLIP_BOX, SKEL_INSTALL, SKEL_FILL_IN = 1, 2, 4
SKEL_OFF, SKEL_ISOLATED, SKEL_END, SKEL_REGULAR, SKEL_JUNCTION = 0, 1, 2, 3, 4
SKEL_LINKS = 13


class VkSkeletonRequest(C.Structure):
    """vk_skeleton_request (32 bytes): the request of vk_skeletonize -- the value range, the mode, the flags, the cap of the iterations
    (0: none), the sample value of a skeleton voxel under SKEL_FILL_IN and of every other voxel."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("mode", C.c_uint32), ("flags", C.c_uint32), ("max_iterations", C.c_uint32), ("fill_in", C.c_float), ("fill_out", C.c_float),
                ("pad", C.c_uint32)]


class VkSkeletonResult(C.Structure):
    """vk_skeleton_result (160 bytes): the totals of vk_skeletonize."""
    _fields_ = [("n_foreground", C.c_uint64), ("n_skeleton", C.c_uint64), ("n_isolated", C.c_uint64), ("n_end", C.c_uint64), ("n_regular", C.c_uint64), ("n_junction", C.c_uint64),
                ("links", C.c_uint64 * SKEL_LINKS), ("iterations", C.c_uint32), ("converged", C.c_uint32)]


assert C.sizeof(VkSkeletonRequest) == 32 and C.sizeof(VkSkeletonResult) == 160


DIFF_OFF, DIFF_MAX_CHECK_EVERY = 0x7FC00000, 1024
DIFF_CLIP_BOX, DIFF_INSTALL = 1, 2


class VkDiffusionRequest(C.Structure):
    """vk_diffusion_request (56 bytes): the request of vk_steady_diffusion -- the value range, the axis (0, 1, 2), the flags, the integer
    spacing per axis (x, y, z), omega (0: automatic), the sweeps per block and the most sweeps, the two stopping bounds, the gain of the
    dense value (0: 1) and the fill of a voxel outside the set."""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("axis", C.c_uint32), ("flags", C.c_uint32), ("spacing", C.c_uint32 * 3), ("omega", C.c_float), ("check_every", C.c_uint32),
                ("max_sweeps", C.c_uint32), ("delta_tol", C.c_float), ("flux_tol", C.c_float), ("gain", C.c_float), ("fill_out", C.c_float)]


class VkDiffusionResult(C.Structure):
    """vk_diffusion_result (80 bytes): the totals of vk_steady_diffusion, the fluxes of its last block as integers, omega and the gain it used."""
    _fields_ = [("n_foreground", C.c_uint64), ("n_inlet", C.c_uint64), ("n_outlet", C.c_uint64), ("n_box", C.c_uint64), ("Fin_q", C.c_int64), ("Fout_q", C.c_int64),
                ("sum_c_q", C.c_int64), ("sweeps", C.c_uint32), ("converged", C.c_uint32), ("delta", C.c_float), ("omega", C.c_float), ("gain", C.c_float), ("pad", C.c_uint32)]


assert C.sizeof(VkDiffusionRequest) == 56 and C.sizeof(VkDiffusionResult) == 80


RESAMPLE_NEAREST, RESAMPLE_LINEAR, RESAMPLE_AREA = 0, 1, 2
RESAMPLE_INSTALL, RESAMPLE_CLIP_BOX, RESAMPLE_WINDOW = 1, 2, 4
RESAMPLE_KEEP_FORMAT = -1
RESAMPLE_MAX_RATIO = 16


class VkResampleRequest(C.Structure):
    """vk_resample_request (36 bytes): the request of vk_volume_resample -- the mode, the flags, the output extents (x, y, z; 0 keeps
    the box's), the output format and layout, the window of the value map."""
    _fields_ = [("mode", C.c_int32), ("flags", C.c_uint32), ("dims", C.c_uint32 * 3), ("format", C.c_int32), ("layout", C.c_int32), ("lo", C.c_float), ("hi", C.c_float)]


class VkResampleResult(C.Structure):
    """vk_resample_result (44 bytes): the output's extents and format, the layout installed (0: none) and the voxel box that was read."""
    _fields_ = [("dims", C.c_uint32 * 3), ("format", C.c_int32), ("layout", C.c_int32), ("box", VkVoxelBox)]


assert C.sizeof(VkResampleRequest) == 36 and C.sizeof(VkResampleResult) == 44


def clip_box(lo, hi) -> VkClipBox:
    """A VkClipBox from two triples, held to vk_set_clip_box's rules before the library sees it: finite components (as f32) and
    0 <= lo < hi <= 1 on every axis.  Raises ValueError."""
    import math

    lo, hi = tuple(float(v) for v in lo), tuple(float(v) for v in hi)
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("clip box: lo and hi need three components each")
    b = VkClipBox()
    for i in range(3):
        if not (math.isfinite(lo[i]) and math.isfinite(hi[i])):
            raise ValueError("clip box: a component is not finite")
        b.lo[i], b.hi[i] = lo[i], hi[i]
        if not 0.0 <= b.lo[i] < b.hi[i] <= 1.0:  # (as the library compares them: rounded to f32)
            raise ValueError("clip box: needs 0 <= lo < hi <= 1 on every axis")
    return b


# every symbol include/vokselis_hip.h declares: name -> (restype, argtypes)
_u32, _i32, _f32, _vp, _sz = C.c_uint32, C.c_int32, C.c_float, C.c_void_p, C.c_size_t
SYMBOLS = {
    "vk_abi_version": (C.c_int, []),
    "vk_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "vk_ctx_destroy": (C.c_int, [_vp]),
    "vk_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "vk_ctx_sync": (C.c_int, [_vp]),
    "vk_device_info": (C.c_int, [_vp, C.c_char_p, _sz, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_sz)]),
    "vk_last_error": (C.c_char_p, [_vp]),
    "vk_volume_upload": (C.c_int, [_vp, _vp, _vp, _u32, _u32, _u32, C.c_int, C.c_int]),
    "vk_volume_upload_device": (C.c_int, [_vp, _vp, _vp, _u32, _u32, _u32, C.c_int, C.c_int]),
    "vk_volume_generate": (C.c_int, [_vp, C.c_int, _u32, _u32, _u32, C.c_int, _u32, _u32, _u32, C.c_int]),
    "vk_volume_generate_xor": (C.c_int, [_vp, _u32, _u32, _u32, _f32]),
    "vk_volume_empty_fraction": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "vk_set_transfer_function": (C.c_int, [_vp, C.POINTER(C.c_float), _u32, _f32, _f32]),
    "vk_set_lighting": (C.c_int, [_vp, _vp]),  # const vk_lighting * (VkLighting below), NULL: off
    "vk_set_projection": (C.c_int, [_vp, C.c_int]),
    "vk_get_projection": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "vk_set_isosurface": (C.c_int, [_vp, _vp]),  # const vk_isosurface * (VkIsosurface above), NULL: off
    "vk_get_isosurface": (C.c_int, [_vp, _vp, C.POINTER(C.c_int)]),
    "vk_set_shadows": (C.c_int, [_vp, _vp]),  # const vk_shadows * (VkShadows above), NULL: off
    "vk_get_shadows": (C.c_int, [_vp, _vp, C.POINTER(C.c_int)]),
    "vk_set_clip_box": (C.c_int, [_vp, _vp]),  # const vk_clip_box * (VkClipBox above), NULL: off
    "vk_get_clip_box": (C.c_int, [_vp, _vp, C.POINTER(C.c_int)]),
    "vk_render_geometry": (C.c_int, [_vp, _i32, _i32, _u32, _u32, _f32, _u32]),
    "vk_geometry_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_vp)]),
    "vk_readback_geometry": (C.c_int, [_vp, _vp, _sz]),
    "vk_frame_geometry": (C.c_int, [_vp, C.c_uint64, _vp, _sz]),
    "vk_pick": (C.c_int, [_vp, _u32, _u32, _f32, _vp]),  # vk_hit * (VkHit above)
    "vk_render_slice": (C.c_int, [_vp, _vp, _i32, _i32, _u32, _u32, _u32]),  # const vk_slice * (VkSlice above)
    "vk_slice_values_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_vp)]),
    "vk_readback_slice_values": (C.c_int, [_vp, _vp, _sz]),
    "vk_frame_slice_values": (C.c_int, [_vp, C.c_uint64, _vp, _sz]),
    "vk_slice_probe": (C.c_int, [_vp, _vp, _u32, _u32, _vp]),  # const vk_slice *, vk_slice_sample * (VkSliceSample above)
    "vk_volume_histogram": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_uint64), _vp]),  # const vk_histogram *, const vk_voxel_box * (NULL: the volume), counts, vk_volume_stats *
    "vk_histogram_window": (C.c_int, [C.POINTER(C.c_uint64), _u32, _f32, _f32, C.c_double, C.c_double, C.POINTER(_f32), C.POINTER(_f32)]),
    "vk_extract_isosurface": (C.c_int, [_vp, _vp, _vp, C.POINTER(_f32), C.c_uint64, C.POINTER(C.c_uint64)]),  # const vk_mesh_request *, const vk_voxel_box * (NULL: the volume), triangles (NULL: count only), cap, n
    "vk_volume_filter": (C.c_int, [_vp, _vp, _vp]),  # const struct vk_volume_filter * (VkVolumeFilter above), dense_out (NULL: install only)
    "vk_filter_gaussian": (C.c_int, [C.c_double, _u32, C.POINTER(_f32)]),
    "vk_label_components": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp]),  # const vk_label_request *, const vk_voxel_box *, labels_out, vk_component *, cap, dense_out, vk_label_result *
    "vk_distance_transform": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),  # const vk_distance_request *, const vk_voxel_box *, d2_out, dense_out, vk_distance_result *
    "vk_split_components": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp]),  # const vk_split_request *, const vk_voxel_box *, labels_out, vk_component *, cap, dense_out, vk_split_result *
    "vk_measure_components": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp]),  # const vk_measure_request *, const vk_voxel_box *, labels_in (NULL: label the range), vk_region *, cap, vk_measure_result *
    "vk_local_thickness": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),  # const vk_thickness_request *, const vk_voxel_box *, t2_out, dense_out, vk_thickness_result *
    "vk_geodesic_distance": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),  # const vk_geodesic_request *, const vk_voxel_box *, g_out, dense_out, vk_geodesic_result *
    "vk_skeletonize": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),  # const vk_skeleton_request *, const vk_voxel_box *, class_out, dense_out, vk_skeleton_result *
    "vk_steady_diffusion": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),  # const vk_diffusion_request *, const vk_voxel_box *, c_out, dense_out, vk_diffusion_result *
    "vk_volume_resample": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),  # const vk_resample_request *, const vk_voxel_box *, dense_out, vk_resample_result *
    "vk_resample_output": (C.c_int, [_vp, _vp, _vp, _vp]),  # const vk_resample_request *, const vk_voxel_box *, vk_resample_result *: the output's extents, format, layout and box, nothing launched
    "vk_volume_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_sz)]),
    "vk_set_uniform": (C.c_int, [_vp, _vp]),
    "vk_set_camera": (C.c_int, [_vp, _vp]),
    "vk_backbuffer_resize": (C.c_int, [_vp, _u32, _u32, C.c_int]),
    "vk_backbuffer_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(C.c_int), C.POINTER(_vp)]),
    "vk_backbuffer_clear": (C.c_int, [_vp]),
    "vk_ctx_frames_in_flight": (C.c_int, [_vp, _u32]),
    "vk_frame_begin": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "vk_frame_end": (C.c_int, [_vp]),
    "vk_frame_wait": (C.c_int, [_vp, C.c_uint64]),
    "vk_frame_readback": (C.c_int, [_vp, C.c_uint64, _vp, _sz]),
    "vk_frame_capture": (C.c_int, [_vp, C.c_uint64, _vp, _sz, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "vk_frame_info": (C.c_int, [_vp, C.c_uint64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int)]),
    "vk_render": (C.c_int, [_vp, C.c_int, _i32, _i32, _u32, _u32, _f32, _u32]),
    "vk_partition_slots": (C.c_int, [_u32, _u32, _u32, _u32, C.POINTER(_u32)]),
    "vk_partition_slots_weighted": (C.c_int, [_u32, _u32, _u32, _u32, _u32, C.POINTER(_u32)]),
    "vk_partition_wire": (C.c_int, [_vp, C.c_int]),
    "vk_wire_pixel_bytes": (C.c_int, [_vp, C.POINTER(_u32)]),
    "vk_tiles_active": (C.c_int, [_vp, C.c_int, _u32, _u32, _u32, C.POINTER(C.c_ubyte), C.POINTER(_u32)]),
    "vk_tiles_active_clip": (C.c_int, [_vp, C.c_int, _u32, _u32, _u32, _vp, C.POINTER(C.c_ubyte), C.POINTER(_u32)]),  # const vk_clip_box *, NULL: the unit cube
    "vk_partition_root_skip": (C.c_int, [_vp, _u32]),
    "vk_render_partition": (C.c_int, [_vp, C.c_int, _u32, _u32, _u32, _f32, _u32, _vp]),
    "vk_partition_order": (C.c_int, [_vp, C.c_int, _u32, C.POINTER(_u32), _u32]),
    "vk_partition_active": (C.c_int, [_vp, C.c_int, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "vk_untile": (C.c_int, [_vp, _vp, _u32, _u32, _u32]),
    "vk_render_batch": (C.c_int, [_vp, C.c_int, _u32, _vp, _u32, _u32, _u32, _f32, _u32, _vp, C.c_int, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "vk_untile_batch": (C.c_int, [_vp, _u32, _vp, _u32, _vp]),
    "vk_untile_batch_over": (C.c_int, [_vp, _u32, _vp, _u32, _vp, _u32]),
    "vk_comm_available": (C.c_int, []),
    "vk_comm_unique_id": (C.c_int, [_vp]),
    "vk_comm_init_rank": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "vk_comm_destroy": (C.c_int, [_vp]),
    "vk_comm_abort": (C.c_int, [_vp]),
    "vk_comm_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vk_gather_tiles": (C.c_int, [_vp, _vp, _vp, _sz, C.c_int, _vp]),
    "vk_group_create": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(_vp)]),
    "vk_group_destroy": (C.c_int, [_vp]),
    "vk_group_size": (C.c_int, [_vp]),
    "vk_group_ctx": (_vp, [_vp, C.c_int]),
    "vk_group_render": (C.c_int, [_vp, C.c_int, _u32, _vp, _u32, _f32, _u32, _vp]),
    "vk_group_sync": (C.c_int, [_vp]),
    "vk_group_peer_direct": (C.c_int, [_vp, C.c_int]),
    "vk_group_last_error": (C.c_char_p, [_vp]),
    "vk_device_alloc": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "vk_device_free": (C.c_int, [_vp, _vp]),
    "vk_device_download": (C.c_int, [_vp, _vp, _vp, _sz]),
    "vk_present": (C.c_int, [_vp, _u32, _u32, C.c_int]),
    "vk_present_info": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_vp), C.POINTER(_vp)]),
    "vk_capture_frame": (C.c_int, [_vp, _vp, _sz, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "vk_readback": (C.c_int, [_vp, _vp, _sz]),
    "vk_step_counts": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vk_step_counts_reset": (C.c_int, [_vp]),
    "vk_simt_census": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "vk_speckle_census": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "vk_debug_set_tile_order": (C.c_int, [_vp, C.POINTER(_u32), _u32]),
    "vk_debug_read_skip_maps": (C.c_int, [_vp, C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_sz), _vp, _sz]),
    "vk_debug_set_param": (C.c_int, [_vp, C.c_char_p, C.c_double]),
    "vk_debug_march_path": (C.c_int, [_vp, C.c_float, _u32, C.POINTER(C.c_int)]),
    "vk_debug_wave_trace": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64), _sz]),
    "vk_readback_steps": (C.c_int, [_vp, _vp]),
    "vk_timer_begin": (C.c_int, [_vp]),
    "vk_timer_end": (C.c_int, [_vp]),
    "vk_timer_elapsed_ms": (C.c_int, [_vp, C.POINTER(_f32)]),
    "vk_dispatch_optimal": (_u32, [_u32, _u32]),
}


class VokselisError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vokselis_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    """Load libvokselis_hip.so; raise (never fall back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback."
            )
        # One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64 / libhsa-runtime64; if this library
        # (linked against /opt/rocm's) is loaded first, a later `import torch` brings a second runtime into the
        # process and whichever initialises second reports "no ROCm-capable device".  Loaded after torch, the
        # dynamic loader resolves this library's libamdhip64.so.7 to the copy already in the process.  Processes
        # that never import torch (the C++ host, a plain C consumer) are unaffected.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the .so does not export it
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(ctx, rc: int):
    if rc != VK_OK:
        msg = lib().vk_last_error(ctx)
        raise VokselisError(rc, msg.decode() if msg else "")
