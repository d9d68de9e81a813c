"""vokselis_amd -- MI355X-native (gfx950) volume raymarcher behind the surface of pudnax/vokselis.

Only the raycast hot path and the host surface that drives it live here:
  csrc/      hand-written HIP kernels + the C-ABI (include/vokselis_hip.h)
  _native    ctypes binding of that C-ABI (fails loudly when the .so is missing)
  camera     Camera / CameraUniform            (src/camera.rs)
  context    Context, Uniform, HdrBackBuffer, VolumeTexture, RaycastPipeline, Demo, run_headless
  volumes    deterministic synthetic volumes (bonsai stand-in, fog)
  slices     Slice: planes for the slice pass (axial / coronal / sagittal / oblique, thick slabs)
  histogram  Histogram: the result of Context.volume_histogram (counts, statistics, percentile window)
  mesh       weld, write_stl, write_obj: the triangles of Context.extract_isosurface as a welded mesh, binary STL, OBJ
  filter     gaussian_weights, filter_request: the weights and the request of Context.filter_volume / smooth_volume / median_volume
  label      Components, label_request, voxel_of: the result and the request of Context.label_components / keep_components
  distance   distance_request, default_fill_in: the request of Context.distance_transform / morph_volume
  split      Regions, split_request: the result and the request of Context.split_components
  measure    Measurements, measure_request: the result and the request of Context.measure_components
  thickness  Thickness, thickness_request: the result and the request of Context.local_thickness
  geodesic   Geodesic, geodesic_request, geodesic_path: the result and the request of Context.geodesic_distance, and the path back to a source
  skeleton   Skeleton, skeleton_request: the result and the request of Context.skeletonize
  diffusion  Diffusion, diffusion_request: the result and the request of Context.steady_diffusion
  resample   resample_request: the request of Context.resample_volume / crop_volume / downsample_volume / isotropic_volume
  dist       tile-parallel multi-GPU frame (one process per GPU, RCCL gather over xGMI)
"""
from . import _native as native
from . import volumes
from ._native import (FMT_R8_UNORM, FMT_R16_FLOAT, FMT_RGBA16F_PAIR, FMT_R16_UNORM, LAYOUT_AUTO, LAYOUT_LINEAR, LAYOUT_PACKED, LAYOUT_PACKED_PAIRS, LAYOUT_BRICKED, LAYOUT_QUADS, LAYOUT_STAGED, RENDER_SAFE, RENDER_FORCE_SKIP,
                      GEN_BONSAI_STANDIN, GEN_FOG, GEN_FOG_DENSE_CORE, MODE_COMPUTE_NEAREST, MODE_NAIVE_TRILINEAR, MODE_PROCEDURAL, OUT_RGBA16F, OUT_RGBA32F, RENDER_COUNT,
                      RENDER_NO_SKIP, RENDER_PROBE_ALWAYS, RENDER_FAST_WALK, RENDER_PRESENT, RENDER_PRESENT_BGRA, RENDER_PRESENT_ONLY, RENDER_DEVICE_SINE, WIRE_RGB, WIRE_RGBA, TF_MAX_ENTRIES, PROJ_COMPOSITE, PROJ_MAX, ISO_MAX_REFINE, VkLighting, VkIsosurface, VkClipBox, VkHit, VokselisError,
                      SLAB_MAX, SLAB_MIN, SLAB_MEAN, SLICE_VALUES, SLICE_MAX_SAMPLES, VkSlice, VkSliceSample,
                      HIST_MAX_BINS, HIST_CLIP_BOX, VkHistogram, VkVoxelBox, VkVolumeStats, MESH_CLIP_BOX, VkMeshRequest,
                      FILTER_MAX_RADIUS, FILTER_MAX_WEIGHT, FILTER_CONVOLVE, FILTER_MEDIAN3, FILTER_INSTALL, VkVolumeFilter,
                      LABEL_MAX_SEEDS, LABEL_KEEP_ALL, LABEL_KEEP_LARGEST, LABEL_KEEP_MIN_SIZE, LABEL_KEEP_SEEDS, LABEL_CLIP_BOX, LABEL_INSTALL, LABEL_INVERT,
                      VkLabelRequest, VkComponent, VkLabelResult,
                      DIST_INF, DIST_MAX_SPACING, DIST_MAX_RADIUS, DIST_OUTSIDE, DIST_INSIDE, DIST_DILATE, DIST_ERODE, DIST_CLOSE, DIST_OPEN, DIST_CLIP_BOX, DIST_INSTALL,
                      VkDistanceRequest, VkDistanceResult,
                      SPLIT_CLIP_BOX, SPLIT_INSTALL, VkSplitRequest, VkSplitResult,
                      MEASURE_CLIP_BOX, VkMeasureRequest, VkRegion, VkMeasureResult,
                      THICK_MAX_REACH, THICK_CLIP_BOX, THICK_INSTALL, VkThicknessRequest, VkThicknessResult,
                      GEO_INF, GEO_FAR, GEO_UNIT, GEO_MAX_SEEDS, GEO_CLIP_BOX, GEO_INSTALL, GEO_FACE_X0, GEO_FACE_X1, GEO_FACE_Y0, GEO_FACE_Y1, GEO_FACE_Z0, GEO_FACE_Z1,
                      VkGeodesicRequest, VkGeodesicResult,
                      SKEL_CURVE, SKEL_KERNEL, SKEL_CLIP_BOX, SKEL_INSTALL, SKEL_FILL_IN, SKEL_OFF, SKEL_ISOLATED, SKEL_END, SKEL_REGULAR, SKEL_JUNCTION, SKEL_LINKS,
                      VkSkeletonRequest, VkSkeletonResult,
                      DIFF_OFF, DIFF_MAX_CHECK_EVERY, DIFF_CLIP_BOX, DIFF_INSTALL, VkDiffusionRequest, VkDiffusionResult,
                      RESAMPLE_NEAREST, RESAMPLE_LINEAR, RESAMPLE_AREA, RESAMPLE_INSTALL, RESAMPLE_CLIP_BOX, RESAMPLE_WINDOW, RESAMPLE_KEEP_FORMAT, RESAMPLE_MAX_RATIO,
                      VkResampleRequest, VkResampleResult)
from .camera import Camera
from .slices import Slice
from .histogram import Histogram
from .mesh import weld, write_obj, write_stl
from .filter import gaussian_weights
from .label import Components, voxel_of
from .distance import distance_request
from .split import Regions, split_request
from .measure import Measurements, measure_request
from .thickness import Thickness, thickness_request
from .geodesic import Geodesic, geodesic_path, geodesic_request
from .skeleton import Skeleton, skeleton_request
from .diffusion import Diffusion, diffusion_request
from .resample import resample_request
from .context import (Context, Demo, FrameCounter, HdrBackBuffer, Hit, ImageDimentions, RaycastPipeline, Uniform,
                      VolumeTexture, dispatch_optimal, partition_slots, render_batch, run_headless, transfer_table, untile_batch)

__all__ = [
    "native", "volumes", "GEN_BONSAI_STANDIN", "GEN_FOG", "GEN_FOG_DENSE_CORE", "Camera", "Context", "Demo", "FrameCounter", "HdrBackBuffer", "ImageDimentions", "RaycastPipeline",
    "Uniform", "VolumeTexture", "dispatch_optimal", "partition_slots", "render_batch", "untile_batch", "run_headless", "transfer_table", "VkLighting", "VokselisError",
    "FMT_R8_UNORM", "FMT_R16_FLOAT", "FMT_RGBA16F_PAIR", "FMT_R16_UNORM", "LAYOUT_AUTO", "LAYOUT_LINEAR", "LAYOUT_PACKED", "LAYOUT_PACKED_PAIRS", "LAYOUT_BRICKED", "LAYOUT_QUADS", "LAYOUT_STAGED", "RENDER_SAFE", "RENDER_FORCE_SKIP",
    "MODE_COMPUTE_NEAREST", "MODE_NAIVE_TRILINEAR", "MODE_PROCEDURAL", "OUT_RGBA16F", "OUT_RGBA32F", "RENDER_COUNT", "RENDER_NO_SKIP", "RENDER_PROBE_ALWAYS", "RENDER_FAST_WALK", "RENDER_PRESENT", "RENDER_PRESENT_BGRA", "RENDER_PRESENT_ONLY", "RENDER_DEVICE_SINE", "WIRE_RGB", "WIRE_RGBA", "TF_MAX_ENTRIES", "PROJ_COMPOSITE", "PROJ_MAX", "ISO_MAX_REFINE", "VkIsosurface", "VkClipBox",
    "VkHit", "Hit",
    "SLAB_MAX", "SLAB_MIN", "SLAB_MEAN", "SLICE_VALUES", "SLICE_MAX_SAMPLES", "VkSlice", "VkSliceSample", "Slice",
    "HIST_MAX_BINS", "HIST_CLIP_BOX", "VkHistogram", "VkVoxelBox", "VkVolumeStats", "Histogram",
    "MESH_CLIP_BOX", "VkMeshRequest", "weld", "write_stl", "write_obj",
    "FILTER_MAX_RADIUS", "FILTER_MAX_WEIGHT", "FILTER_CONVOLVE", "FILTER_MEDIAN3", "FILTER_INSTALL", "VkVolumeFilter", "gaussian_weights",
    "LABEL_MAX_SEEDS", "LABEL_KEEP_ALL", "LABEL_KEEP_LARGEST", "LABEL_KEEP_MIN_SIZE", "LABEL_KEEP_SEEDS", "LABEL_CLIP_BOX", "LABEL_INSTALL", "LABEL_INVERT",
    "VkLabelRequest", "VkComponent", "VkLabelResult", "Components", "voxel_of",
    "DIST_INF", "DIST_MAX_SPACING", "DIST_MAX_RADIUS", "DIST_OUTSIDE", "DIST_INSIDE", "DIST_DILATE", "DIST_ERODE", "DIST_CLOSE", "DIST_OPEN", "DIST_CLIP_BOX", "DIST_INSTALL",
    "VkDistanceRequest", "VkDistanceResult", "distance_request",
    "SPLIT_CLIP_BOX", "SPLIT_INSTALL", "VkSplitRequest", "VkSplitResult", "Regions", "split_request",
    "MEASURE_CLIP_BOX", "VkMeasureRequest", "VkRegion", "VkMeasureResult", "Measurements", "measure_request",
    "THICK_MAX_REACH", "THICK_CLIP_BOX", "THICK_INSTALL", "VkThicknessRequest", "VkThicknessResult", "Thickness", "thickness_request",
    "GEO_INF", "GEO_FAR", "GEO_UNIT", "GEO_MAX_SEEDS", "GEO_CLIP_BOX", "GEO_INSTALL", "GEO_FACE_X0", "GEO_FACE_X1", "GEO_FACE_Y0", "GEO_FACE_Y1", "GEO_FACE_Z0", "GEO_FACE_Z1",
    "VkGeodesicRequest", "VkGeodesicResult", "Geodesic", "geodesic_request", "geodesic_path",
    "SKEL_CURVE", "SKEL_KERNEL", "SKEL_CLIP_BOX", "SKEL_INSTALL", "SKEL_FILL_IN", "SKEL_OFF", "SKEL_ISOLATED", "SKEL_END", "SKEL_REGULAR", "SKEL_JUNCTION", "SKEL_LINKS",
    "VkSkeletonRequest", "VkSkeletonResult", "Skeleton", "skeleton_request",
    "DIFF_OFF", "DIFF_MAX_CHECK_EVERY", "DIFF_CLIP_BOX", "DIFF_INSTALL", "VkDiffusionRequest", "VkDiffusionResult", "Diffusion", "diffusion_request",
    "RESAMPLE_NEAREST", "RESAMPLE_LINEAR", "RESAMPLE_AREA", "RESAMPLE_INSTALL", "RESAMPLE_CLIP_BOX", "RESAMPLE_WINDOW", "RESAMPLE_KEEP_FORMAT", "RESAMPLE_MAX_RATIO",
    "VkResampleRequest", "VkResampleResult", "resample_request",
]
