"""The refusals the slice, histogram, mesh and filter entry points share (vk_launch.hpp: pass_needs, pass_voxel_box), on the MI355X: the
full error text and the status of each, as the entry points spelled them before they shared the code, and after every refusal a valid
call on the same context that still gives the known result -- counts that sum to the 512 voxels, the restatement's triangle count."""
import ctypes as C

import numpy as np
import pytest

import mesh_helpers as MH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
PASSES = ("slice", "histogram", "mesh", "filter")
NO_VOLUME = {"slice": "vk_render_slice: no volume uploaded", "histogram": "vk_volume_histogram: no volume uploaded",
             "mesh": "vk_extract_isosurface: no volume uploaded", "filter": "vk_volume_filter: no volume uploaded"}
NO_KERNELS = {
    "slice": "slice: the slice pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no slice kernels)",
    "histogram": "histogram: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no histogram kernels)",
    "mesh": "mesh: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no mesh kernels)",
    "filter": "filter: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no filter kernels)"}
BOX_NOT_NULL = {"histogram": "vk_volume_histogram: VK_HIST_CLIP_BOX takes the box from the clip box: box must be NULL",
                "mesh": "vk_extract_isosurface: VK_MESH_CLIP_BOX takes the box from the clip box: box must be NULL"}
BOX_BAD = {"histogram": "vk_volume_histogram: the box is inverted or leaves the volume", "mesh": "vk_extract_isosurface: the box is inverted or leaves the volume"}
SIZE = (16, 16)


@pytest.fixture(scope="module")
def vol():
    v = np.random.default_rng(13).integers(0, 256, (8, 8, 8)).astype(np.uint8)
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def n_triangles(vol, tmp_path_factory):
    return len(MH.restate(MH.build_restatement(tmp_path_factory.mktemp("pass_refusals")), vol, "u8", 0.5))


def _call(V, ctx, name, box=None, clip_flag=False):
    """The pass through its C entry point with a valid request: (status, vk_last_error)."""
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
    else:
        out = np.zeros(512, np.uint8)
        r = N.VkVolumeFilter()
        r.radius[0] = 1
        r.weights[0][0], r.weights[0][1], r.weights[0][2] = 0.25, 0.5, 0.25
        rc = L.vk_volume_filter(ctx.handle, C.byref(r), out.ctypes.data)
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
        for name in ("histogram", "mesh"):
            assert _call(V, ctx, name, (0, 0, 0, 1, 1, 1), clip_flag=True) == (INVALID, BOX_NOT_NULL[name]), name
            assert _still_good(V, ctx, n_triangles), name
            for box in ((2, 0, 0, 1, 1, 1), (0, 0, 0, 9, 1, 1), (0, 0, 8, 1, 1, 9)):  # inverted; leaves the volume
                assert _call(V, ctx, name, box) == (INVALID, BOX_BAD[name]), (name, box)
                assert _still_good(V, ctx, n_triangles), (name, box)
    finally:
        ctx.close()
