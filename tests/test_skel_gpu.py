"""vk_skeletonize on the MI355X, in use: VK_SKEL_INSTALL followed by the passes that read the volume --
vk_volume_histogram counts exactly what the restatement's dense array predicts, and a table render of it stays finite; an install
leaves table, projection, isosurface, lighting and clip box in force; the Python wrapper with its derived values; the C++ host's
bonsai --skeleton on the fixed bar."""
import math
import os
import subprocess

import numpy as np
import pytest

import dist_cases as DC
import label_helpers as LH
import skel_cases as SC
import skel_helpers as SH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID = -1
W, H = 64, 64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("skel_gpu"))


def _ctx(V):  # noqa: F811
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    return V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)


def _table(V):  # noqa: F811
    return V.transfer_table([(0.0, 0.0, 0.0, 0.0, 0.0), (0.3, 0.1, 0.2, 0.9, 0.0), (0.5, 1.0, 0.5, 0.1, 0.4), (1.0, 1.0, 1.0, 1.0, 0.9)], 64)


def _frame(V, ctx):  # noqa: F811
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
    return ctx.read_backbuffer().copy()


def _held(ctx):
    """The volume the context holds, as a dense array."""
    return ctx.keep_components(-math.inf, math.inf, keep="all", install=False, out=True)[0]


def _bar(kind="u8"):
    return DC.mask_volume(SC.fixed_bar(), kind)


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED"), ("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_install_then_histogram_and_a_table_render_read_the_skeleton(V, lib, kind, layout):  # noqa: F811
    """The fixed bar in curve mode: the installed volume is the restatement's dense array bit for bit, its histogram is that of a fresh
    upload of that array, and the table march renders it to finite pixels."""
    vol = _bar(kind)
    cls, dense, result = SH.restate(lib, vol, kind, 0.5, math.inf, SC.CURVE, fill_in=0.5)
    assert [int(v) for v in result[:6]] == [650, 26, 0, 5, 20, 1]
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
        info = ctx._volume_dtype()
        k = ctx.skeletonize(0.5, fill_in=0.5, install=True, classes=True, out=True)
        assert (k.classes == cls).all() and (LH.raw(k.dense) == LH.raw(dense)).all() and (SH.result_array(k_result(k)) == result).all()
        assert (k.n_skeleton, k.n_end, k.n_junction, k.n_isolated, k.iterations, k.converged) == (26, 5, 1, 0, 2, True) and ctx._volume_dtype() == info
        assert (LH.raw(_held(ctx)) == LH.raw(dense)).all()                                          # ... and it was installed
        fresh = _ctx(V)
        try:
            LH.upload(V, fresh, dense, kind, layout)
            fresh.update()
            want = np.asarray(fresh.volume_histogram(64, (0.0, 1.0)).counts)
        finally:
            fresh.close()
        counts = np.asarray(ctx.volume_histogram(64, (0.0, 1.0)).counts)
        assert (counts == want).all() and int(counts.sum()) == vol.size and int(counts[0]) == vol.size - 26   # every voxel off the skeleton stores 0
        ctx.set_transfer_function(_table(V), (0.0, 1.0))
        frame = _frame(V, ctx)
        assert np.isfinite(frame).all() and np.abs(frame[..., :3]).sum() > 0
    finally:
        ctx.close()


def k_result(k):
    """A Skeleton's totals as the struct the helpers compare."""
    import ctypes as C

    import vokselis_amd as V  # noqa: F811

    return V.VkSkeletonResult(k.n_foreground, k.n_skeleton, k.n_isolated, k.n_end, k.n_regular, k.n_junction, (C.c_uint64 * 13)(*k.links), k.iterations, int(k.converged))


STATES = {
    "table, lighting, clip box": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_lighting((0.3, 0.5, 0.8)), c.set_clip_box((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))),
    "table, max projection": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_projection("max")),
    "isosurface": lambda V, c: c.set_isosurface(0.35, (0.9, 0.8, 0.7), 4),
}


@pytest.mark.parametrize("state", sorted(STATES))
def test_an_install_leaves_table_projection_isosurface_lighting_and_clip_box_in_force(V, lib, state):  # noqa: F811
    """Context a installs the skeleton under the state; context b gets the same state and a fresh upload of the restatement's dense array:
    the two render the same frame bit for bit, which they would not if the install had dropped any of the state."""
    c = next(c for c in SC.cases() if c.kind == "u8" and "density 0.9" in c.name and c.box is None and c.max_iterations == 0)
    dense = SH.restate_case(lib, c)[1]
    a, b = _ctx(V), _ctx(V)
    try:
        for ctx in (a, b):
            STATES[state](V, ctx)
        in_force = (a.isosurface, a.clip_box, a.projection)
        LH.upload(V, a, c.vol, "u8", "PACKED")
        LH.upload(V, b, dense, "u8", "PACKED")
        a.update()
        b.update()
        before = _frame(V, a)
        k = a.skeletonize(c.lo, c.hi, mode=SC.MODE_NAME[c.mode], fill_in=c.fill_in, fill_out=c.fill_out)   # install is the default
        assert k.converged and 0 < k.n_skeleton < k.n_foreground and k.dense is None and k.classes is None
        assert (a.isosurface, a.clip_box, a.projection) == in_force == (b.isosurface, b.clip_box, b.projection)
        fa, fb = _frame(V, a), _frame(V, b)
        assert (fa.view(np.uint32) == fb.view(np.uint32)).all() and np.isfinite(fa).all() and np.abs(fa[..., :3]).sum() > 0
        assert not (fa.view(np.uint32) == before.view(np.uint32)).all()                             # the skeleton is not the volume it came from
        assert (_held(a) == dense).all()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_python_wrapper_against_the_restatement(V, lib, kind, layout):  # noqa: F811
    import label_cases as LC

    d = (33, 9, 10)
    vol = LC.noise(d, kind, 12)
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
        info = ctx._volume_dtype()
        want = SH.restate(lib, vol, kind, 0.3, math.inf, SC.CURVE)
        k = ctx.skeletonize(0.3, install=False, classes=True, out=True)                             # the defaults: curve mode, to convergence, stored values kept, 0 elsewhere
        assert k.classes.dtype == np.uint8 and k.dense.dtype == vol.dtype and SH.differences((k.classes, k.dense, SH.result_array(k_result(k))), want) == ""
        assert k.converged and k.n_skeleton == int((k.classes != 0).sum()) == k.n_isolated + k.n_end + k.n_regular + k.n_junction
        assert k.length() == pytest.approx(sum(n * math.sqrt(dx * dx + dy * dy + dz * dz) for n, (dx, dy, dz) in zip(k.links, V.skeleton.link_offsets())), rel=1e-15) and k.length() > 0
        assert (LH.raw(_held(ctx)) == LH.raw(np.ascontiguousarray(vol))).all() and ctx._volume_dtype() == info   # not installed
        totals = ctx.skeletonize(0.3, install=False)
        assert totals.classes is None and totals.dense is None and (SH.result_array(k_result(totals)) == want[2]).all()
        box = ((3, 1, 1), (30, 9, 7))
        want = SH.restate(lib, vol, kind, 0.2, 0.8, SC.KERNEL, 3, 0.75, 0.25, box[0] + box[1])
        k = ctx.skeletonize(0.2, 0.8, mode="kernel", max_iterations=3, fill_in=0.75, fill_out=0.25, box=box, install=False, classes=True, out=True)
        assert SH.differences((k.classes, k.dense, SH.result_array(k_result(k))), want) == "" and not k.converged and k.iterations == 3
        clip = ((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
        ctx.set_clip_box(*clip)
        k = ctx.skeletonize(0.3, mode="kernel", box="clip", install=False, classes=True)
        ctx.set_clip_box(None)
        want = SH.restate(lib, vol, kind, 0.3, math.inf, SC.KERNEL, box=LC.clip_voxel_box(clip[0], clip[1], d))
        assert (k.classes == want[0]).all() and (SH.result_array(k_result(k)) == want[2]).all()
        want = SH.restate(lib, vol, kind, 0.3, math.inf, SC.CURVE, fill_out=0.5)
        k = ctx.skeletonize(0.3, fill_out=0.5)
        assert (SH.result_array(k_result(k)) == want[2]).all() and (LH.raw(_held(ctx)) == LH.raw(want[1])).all() and ctx._volume_dtype() == info
        for bad in (dict(mode="surface"), dict(max_iterations=-1)):
            with pytest.raises(ValueError):
                ctx.skeletonize(0.3, **bad)
        with pytest.raises(V.VokselisError) as e:
            ctx.skeletonize(0.3, fill_out=math.inf, install=False)
        assert e.value.code == INVALID and "fill_out is not finite" in str(e.value)
    finally:
        ctx.close()


def _bonsai():
    import __graft_entry__ as g

    g.build_host()
    return os.path.join(LH.ROOT, "vokselis_amd", "_lib", "bonsai")


@pytest.mark.parametrize("kind, mode", [("u8", "curve"), ("u16", "kernel")])
def test_bonsai_skeleton_writes_the_restatements_volume_of_the_fixed_bar(V, lib, tmp_path, kind, mode):  # noqa: F811
    """bonsai --skeleton --save-raw on the fixed bar: the saved file is the restatement's dense array, bit for bit, and the counts and the
    length are printed."""
    vol = _bar(kind)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [_bonsai(), "--raw-u16" if kind == "u16" else "--raw", str(src), "--dims", "26", "5", "5", "--components", "0.5", "inf", "--skeleton", mode, "--morph-spacing", "1", "2", "3",
            "--label-fill", "0.25", "--save-raw", str(dst), "--histogram", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = SH.restate(lib, vol, kind, 0.5, math.inf, SC.CURVE if mode == "curve" else SC.KERNEL, fill_out=0.25)
    n = [int(v) for v in want[2]]
    import vokselis_amd as VA

    length = sum(c * math.sqrt(dx * dx + 4 * dy * dy + 9 * dz * dz) for c, (dx, dy, dz) in zip(n[SH.R_LINKS:SH.R_LINKS + 13], VA.skeleton.link_offsets()))
    line = "skeleton: [0.5, inf] %s spacing 1 2 3: 650 foreground voxels, %d skeleton voxels, %d ends, %d junctions, %d isolated voxels, length %.6g, %d iterations" % (
        mode, n[1], n[3], n[5], n[2], length, n[SH.R_ITERATIONS])
    assert line in r.stdout.splitlines(), r.stdout[-800:]
    assert (n[1], n[3], n[5]) == ((26, 5, 1) if mode == "curve" else (1, 0, 0))
    got = np.fromfile(dst, vol.dtype).reshape(vol.shape)
    assert SH.differences((None, got, None), (None, want[1], None)) == ""


def test_bonsai_skeleton_stops_at_max_iter_and_says_so(V, lib, tmp_path):  # noqa: F811
    vol = DC.mask_volume(SC.ball(), "u8")
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [_bonsai(), "--raw", str(src), "--dims"] + [str(v) for v in SC.SHAPES] + ["--iso", "0.5", "--skeleton", "kernel", "2", "--save-raw", str(dst), "--histogram", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = SH.restate(lib, vol, "u8", 0.5, math.inf, SC.KERNEL, 2)
    assert "%d skeleton voxels" % int(want[2][1]) in r.stdout and "2 iterations (stopped by MAX_ITER)" in r.stdout, r.stdout[-800:]
    assert (np.fromfile(dst, np.uint8).reshape(vol.shape) == want[1]).all()
