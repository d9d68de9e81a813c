"""The refusals the entry points of the passes that are not a march share (vk_launch.hpp: pass_needs, pass_voxel_box,
pass_install_refused), on the MI355X: the full error text and the status of each, as the entry points spelled them before they shared the
code, and after every refusal a valid call on the same context that still gives the known result -- counts that sum to the 512 voxels,
the restatement's triangle count."""
import ctypes as C

import numpy as np
import pytest

import mesh_helpers as MH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
PASSES = ("slice", "histogram", "mesh", "filter", "label", "distance", "split", "resample")
BOX_PASSES = ("histogram", "mesh", "label", "distance", "split", "resample")
NO_VOLUME = {"slice": "vk_render_slice: no volume uploaded", "histogram": "vk_volume_histogram: no volume uploaded",
             "mesh": "vk_extract_isosurface: no volume uploaded", "filter": "vk_volume_filter: no volume uploaded",
             "label": "vk_label_components: no volume uploaded", "distance": "vk_distance_transform: no volume uploaded",
             "split": "vk_split_components: no volume uploaded", "resample": "resample: no volume uploaded"}
NO_KERNELS = {
    "slice": "slice: the slice pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no slice kernels)",
    "histogram": "histogram: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no histogram kernels)",
    "mesh": "mesh: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no mesh kernels)",
    "filter": "filter: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no filter kernels)",
    "label": "label: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no label kernels)",
    "distance": "distance: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no distance kernels)",
    "split": "split: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no split kernels)",
    "resample": "resample: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no resample kernels)"}
BOX_NOT_NULL = {"histogram": "vk_volume_histogram: VK_HIST_CLIP_BOX takes the box from the clip box: box must be NULL",
                "mesh": "vk_extract_isosurface: VK_MESH_CLIP_BOX takes the box from the clip box: box must be NULL",
                "label": "vk_label_components: VK_LABEL_CLIP_BOX takes the box from the clip box: box must be NULL",
                "distance": "vk_distance_transform: VK_DIST_CLIP_BOX takes the box from the clip box: box must be NULL",
                "split": "vk_split_components: VK_SPLIT_CLIP_BOX takes the box from the clip box: box must be NULL",
                "resample": "resample: VK_RESAMPLE_CLIP_BOX takes the box from the clip box: box must be NULL"}
BOX_BAD = {"histogram": "vk_volume_histogram: the box is inverted or leaves the volume", "mesh": "vk_extract_isosurface: the box is inverted or leaves the volume",
           "label": "vk_label_components: the box is inverted or leaves the volume", "distance": "vk_distance_transform: the box is inverted or leaves the volume",
           "split": "vk_split_components: the box is inverted or leaves the volume", "resample": "resample: the box is inverted or leaves the volume"}
INSTALL_WHILE_RECORDING = {
    "filter": "vk_volume_filter: VK_FILTER_INSTALL while a frame is being recorded (call it outside vk_frame_begin / vk_frame_end)",
    "label": "vk_label_components: VK_LABEL_INSTALL while a frame is being recorded (call it outside vk_frame_begin / vk_frame_end)",
    "distance": "vk_distance_transform: VK_DIST_INSTALL while a frame is being recorded (call it outside vk_frame_begin / vk_frame_end)",
    "split": "vk_split_components: VK_SPLIT_INSTALL while a frame is being recorded (call it outside vk_frame_begin / vk_frame_end)",
    "resample": "resample: VK_RESAMPLE_INSTALL while a frame is being recorded (call it outside vk_frame_begin / vk_frame_end)"}
SIZE = (16, 16)


@pytest.fixture(scope="module")
def vol():
    v = np.random.default_rng(13).integers(0, 256, (8, 8, 8)).astype(np.uint8)
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def n_triangles(vol, tmp_path_factory):
    return len(MH.restate(MH.build_restatement(tmp_path_factory.mktemp("pass_refusals")), vol, "u8", 0.5))


def _call(V, ctx, name, box=None, clip_flag=False, install=False):
    """The pass through its C entry point with a valid request: (status, vk_last_error).  install (filter, label, distance, split,
    resample): the request installs and asks for nothing else, else it writes into host arrays that are thrown away."""
    from vokselis_amd.distance import distance_request
    from vokselis_amd.label import label_request
    from vokselis_amd.resample import resample_request
    from vokselis_amd.split import split_request

    N, L = V.native, V.native.lib()
    b = C.byref(N.VkVoxelBox(*box)) if box is not None else None
    if name == "slice":
        s = V.Slice.raw((0.1, 0.1, 0.5), (0.05, 0.0, 0.0), (0.0, 0.05, 0.0), (0.0, 0.0, 0.05), 1, "max")
        rc = L.vk_render_slice(ctx.handle, C.byref(s), 0, 0, SIZE[0], SIZE[1], 0)
    elif name == "histogram":
        rc = L.vk_volume_histogram(ctx.handle, C.byref(N.VkHistogram(0.0, 1.0, 256, N.HIST_CLIP_BOX if clip_flag else 0)), b, None, None)
    elif name == "mesh":
        n = C.c_uint64(0)
        rc = L.vk_extract_isosurface(ctx.handle, C.byref(N.VkMeshRequest(0.5, N.MESH_CLIP_BOX if clip_flag else 0)), b, None, 0, C.byref(n))
    elif name == "filter":
        out = np.zeros(512, np.uint8)
        r = N.VkVolumeFilter()
        r.flags = N.FILTER_INSTALL if install else 0
        r.radius[0] = 1
        r.weights[0][0], r.weights[0][1], r.weights[0][2] = 0.25, 0.5, 0.25
        rc = L.vk_volume_filter(ctx.handle, C.byref(r), None if install else out.ctypes.data)
    elif name == "label":
        r, res = label_request(0.5, keep="largest", box="clip" if clip_flag else None, install=install), N.VkLabelResult()
        rc = L.vk_label_components(ctx.handle, C.byref(r), b, None, None, 0, None, C.byref(res))
    elif name == "distance":
        d2, res = np.zeros(512, np.uint32), N.VkDistanceResult()
        if install:
            r = distance_request(0.5, op="close", radius=1.0, box="clip" if clip_flag else None, install=True)
            rc = L.vk_distance_transform(ctx.handle, C.byref(r), b, None, None, C.byref(res))
        else:
            rc = L.vk_distance_transform(ctx.handle, C.byref(distance_request(0.5, box="clip" if clip_flag else None)), b, d2.ctypes.data, None, None)
    elif name == "split":
        r, res = split_request(0.5, radius=1.0, box="clip" if clip_flag else None, install=install), N.VkSplitResult()
        rc = L.vk_split_components(ctx.handle, C.byref(r), b, None, None, 0, None, C.byref(res))
    else:
        out, res = np.zeros(512, np.uint8), N.VkResampleResult()
        r = resample_request(None, "nearest", box="clip" if clip_flag else None, install=install, out=not install)
        rc = L.vk_volume_resample(ctx.handle, C.byref(r), b, None if install else out.ctypes.data, C.byref(res))
    return rc, L.vk_last_error(ctx.handle).decode()


def _still_good(V, ctx, n_triangles):
    h = ctx.volume_histogram(256, (0.0, 1.0))
    return int(h.counts.sum()) == 512 and h.n_voxels == 512 and len(ctx.extract_isosurface(0.5)) == n_triangles


def _refused_then_good(V, ctx, vol, n_triangles, expected, status):
    """Every pass is refused with its text; then the context takes a PACKED volume and every pass works on it."""
    for name in PASSES:
        assert _call(V, ctx, name) == (status, expected[name]), name
    V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
    assert _still_good(V, ctx, n_triangles)
    for name in PASSES:
        assert _call(V, ctx, name)[0] == 0, name
    assert _still_good(V, ctx, n_triangles)


def test_no_volume_uploaded(V, vol, n_triangles):  # noqa: F811
    ctx = V.Context(SIZE[0], SIZE[1], backbuffer=SIZE, out_format=V.OUT_RGBA32F)
    try:
        _refused_then_good(V, ctx, vol, n_triangles, NO_VOLUME, INVALID)
    finally:
        ctx.close()


def test_a_bricked_volume_has_no_kernels(V, vol, n_triangles):  # noqa: F811
    ctx = V.Context(SIZE[0], SIZE[1], backbuffer=SIZE, out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, vol, layout=V.LAYOUT_BRICKED)
        _refused_then_good(V, ctx, vol, n_triangles, NO_KERNELS, UNSUPPORTED)
    finally:
        ctx.close()


def test_a_pair_volume_has_no_kernels(V, vol, n_triangles):  # noqa: F811
    ctx = V.Context(SIZE[0], SIZE[1], backbuffer=SIZE, out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))  # RGBA16F_PAIR
        _refused_then_good(V, ctx, vol, n_triangles, NO_KERNELS, UNSUPPORTED)
    finally:
        ctx.close()


def test_the_box_refusals_of_histogram_and_mesh(V, vol, n_triangles):  # noqa: F811
    ctx = V.Context(SIZE[0], SIZE[1], backbuffer=SIZE, out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
        assert _still_good(V, ctx, n_triangles)
        for name in BOX_PASSES:
            assert _call(V, ctx, name, (0, 0, 0, 1, 1, 1), clip_flag=True) == (INVALID, BOX_NOT_NULL[name]), name
            assert _still_good(V, ctx, n_triangles), name
            for box in ((2, 0, 0, 1, 1, 1), (0, 0, 0, 9, 1, 1), (0, 0, 8, 1, 1, 9)):  # inverted; leaves the volume
                assert _call(V, ctx, name, box) == (INVALID, BOX_BAD[name]), (name, box)
                assert _still_good(V, ctx, n_triangles), (name, box)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sorted(INSTALL_WHILE_RECORDING))
def test_an_install_while_a_frame_is_recorded(V, vol, n_triangles, name):  # noqa: F811
    """Between frame_begin and frame_end the installing call is refused with its text; the frame still ends and reads back, the volume is
    the one uploaded, and the same call installs once the frame is over: the volume keeps its 512 voxels."""
    ctx = V.Context(SIZE[0], SIZE[1], backbuffer=SIZE, out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
        assert _call(V, ctx, "slice")[0] == 0
        before = ctx.read_backbuffer().copy()
        fid = ctx.frame_begin()
        assert _call(V, ctx, "slice")[0] == 0
        refused = _call(V, ctx, name, install=True)
        ctx.frame_end()
        assert refused == (INVALID, INSTALL_WHILE_RECORDING[name])
        assert (ctx.read_frame(fid).view(np.uint32) == before.view(np.uint32)).all()
        assert _still_good(V, ctx, n_triangles)
        assert _call(V, ctx, name, install=True)[0] == 0
        h = ctx.volume_histogram(256, (0.0, 1.0))
        assert int(h.counts.sum()) == 512 and h.n_voxels == 512
        assert _call(V, ctx, name)[0] == 0
    finally:
        ctx.close()
