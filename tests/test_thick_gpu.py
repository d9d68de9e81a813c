"""vk_local_thickness on the MI355X, in use: VK_THICK_INSTALL followed by the passes that read the map --
vk_volume_histogram gives the thickness distribution, vk_measure_components with a label array the sum of the stored values per region,
both exactly what the restatement's dense array predicts; an install leaves table, projection, isosurface, lighting and clip box in
force; the Python wrapper; the C++ host's bonsai --thickness on the issue's fixed case."""
import math
import os
import subprocess

import numpy as np
import pytest

import dist_cases as DC
import label_helpers as LH
import thick_cases as TC
import thick_helpers as TH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID = -1
W, H = 64, 64


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("thick_gpu")
    return TH.build_restatement(d), LH.build_restatement(d)


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


def _fixed(kind="u8"):
    d, A, B = TC.fixed_case()
    return DC.mask_volume(A | B, kind), A, B


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED"), ("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_install_then_histogram_and_measure_read_the_thickness_map(V, libs, kind, layout):  # noqa: F811
    """The fixed case at cap 6: the installed map is the restatement's dense array bit for bit; its histogram is the thickness
    distribution; measured with the components' labels, sum_q over a region is the sum of the stored values the restatement predicts."""
    vol, A, B = _fixed(kind)
    t2, dense, result = TH.restate(libs[0], vol, kind, 0.5, math.inf, (1, 1, 1), 6.0)
    assert int(result[0]) == 3586 and int(result[1]) == 36 and int(result[2]) == 3017
    labels = LH.restate(libs[1], vol, kind, 0.5, math.inf, 6)[0]
    assert int(labels.max()) == 1
    labels = np.where(B & ~A, np.uint32(2), labels).astype(np.uint32)  # two regions by the caller's segmentation: ball A, and what B adds
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
        info = ctx._volume_dtype()
        t = ctx.local_thickness(0.5, max_radius=6.0, install=True, out=True, t2=True)
        assert (t.t2 == t2).all() and (LH.raw(t.dense) == LH.raw(dense)).all() and (TH.result_array(t) == result).all()
        assert t.max_thickness == 12.0 and t.mean_t2 == int(result[3]) / 3586 and ctx._volume_dtype() == info
        assert (LH.raw(_held(ctx)) == LH.raw(dense)).all()                                          # ... and it was installed
        # the distribution: the histogram of the installed map is that of a fresh upload of the restatement's array; three distinct T2 (26 on B outside A,
        # A's rim, and the cap) and the fill, each in a bin of its own
        fresh = _ctx(V)
        try:
            LH.upload(V, fresh, dense, kind, layout)
            fresh.update()
            want = np.asarray(fresh.volume_histogram(64, (0.0, 1.0)).counts)
        finally:
            fresh.close()
        counts = np.asarray(ctx.volume_histogram(64, (0.0, 1.0)).counts)
        assert (counts == want).all() and int(counts[0]) == vol.size - 3586 and int((counts > 0).sum()) == 4 and int(counts.max()) == vol.size - 3586
        assert sorted(int(c) for c in counts[counts > 0])[-2] == 3017                               # the saturated voxels, at full scale
        # the sum of the stored values per region
        m = ctx.measure_components(labels=labels)
        q = LH.raw(dense).astype(np.int64) if kind != "f16" else np.rint(dense.astype(np.float64) * 2.0 ** 24).astype(np.int64)
        assert m.n == 2 and [int(s) for s in m.sizes] == [3586 - 515, 515]
        assert [int(s) for s in m.sum_q] == [int(q[labels == 1].sum()), int(q[labels == 2].sum())]
        assert int(q[labels == 2].min()) == int(q[labels == 2].max())                               # every voxel of B outside A holds the one value: T2 = 26
    finally:
        ctx.close()


STATES = {
    "table, lighting, clip box": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_lighting((0.3, 0.5, 0.8)), c.set_clip_box((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))),
    "table, max projection": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_projection("max")),
    "isosurface": lambda V, c: c.set_isosurface(0.35, (0.9, 0.8, 0.7), 4),
}


@pytest.mark.parametrize("state", sorted(STATES))
def test_an_install_leaves_table_projection_isosurface_lighting_and_clip_box_in_force(V, libs, state):  # noqa: F811
    """Context a installs the thickness map under the state; context b gets the same state and a fresh upload of the restatement's map:
    the two render the same frame bit for bit, which they would not if the install had dropped any of the state."""
    vol, _, _ = _fixed("u8")
    dense = TH.restate(libs[0], vol, "u8", 0.5, math.inf, (1, 1, 1), 32.0)[1]
    a, b = _ctx(V), _ctx(V)
    try:
        for ctx in (a, b):
            STATES[state](V, ctx)
        in_force = (a.isosurface, a.clip_box, a.projection)
        LH.upload(V, a, vol, "u8", "PACKED")
        LH.upload(V, b, dense, "u8", "PACKED")
        a.update()
        b.update()
        before = _frame(V, a)
        t = a.local_thickness(0.5, max_radius=32.0, install=True)
        assert t.max_t2 == 82 and t.n_saturated == 0 and t.dense is None and t.t2 is None
        assert (a.isosurface, a.clip_box, a.projection) == in_force == (b.isosurface, b.clip_box, b.projection)
        fa, fb = _frame(V, a), _frame(V, b)
        assert (fa.view(np.uint32) == fb.view(np.uint32)).all() and np.abs(fa[..., :3]).sum() > 0
        assert state == "isosurface" or not (fa.view(np.uint32) == before.view(np.uint32)).all()                             # the map is not the volume it came from
        assert (_held(a) == dense).all()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_python_wrapper_against_the_restatement(V, libs, kind, layout):  # noqa: F811
    import label_cases as LC

    vol = LC.noise((33, 9, 10), kind, 12)
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
        info = ctx._volume_dtype()
        want = TH.restate(libs[0], vol, kind, 0.3, math.inf, (1, 1, 1), 16.0)
        t = ctx.local_thickness(0.3, out=True, t2=True)                                             # the defaults: cap 16, spacing 1, automatic gain, no install
        assert t.t2.dtype == np.uint32 and t.dense.dtype == vol.dtype and TH.differences((t.t2, t.dense, TH.result_array(t)), want) == ""
        assert t.gain == float(np.float32(1.0) / np.sqrt(np.float32(t.max_t2))) and t.max_thickness == 2.0 * math.sqrt(t.max_t2)
        assert (LH.raw(_held(ctx)) == LH.raw(np.ascontiguousarray(vol))).all() and ctx._volume_dtype() == info   # not installed
        totals = ctx.local_thickness(0.3)
        assert totals.t2 is None and totals.dense is None and (TH.result_array(totals) == want[2]).all()
        box = ((2, 1, 0), (30, 9, 7))
        want = TH.restate(libs[0], vol, kind, 0.2, 0.8, (2, 2, 5), 9.0, 0.125, 0.25, box[0] + box[1])
        t = ctx.local_thickness(0.2, 0.8, max_radius=9.0, spacing=(2, 2, 5), box=box, gain=0.125, fill_out=0.25, out=True, t2=True)
        assert TH.differences((t.t2, t.dense, TH.result_array(t)), want) == "" and t.gain == 0.125
        clip = ((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
        ctx.set_clip_box(*clip)
        t = ctx.local_thickness(0.3, max_radius=4.0, box="clip", t2=True)
        ctx.set_clip_box(None)
        assert (t.t2 == TH.restate(libs[0], vol, kind, 0.3, math.inf, (1, 1, 1), 4.0, box=LC.clip_voxel_box(clip[0], clip[1], (33, 9, 10)))[0]).all()
        want = TH.restate(libs[0], vol, kind, 0.3, math.inf, (3, 1, 2), 5.0, 0.2)
        t = ctx.local_thickness(0.3, max_radius=5.0, spacing=(3, 1, 2), gain=0.2, install=True)
        assert (TH.result_array(t) == want[2]).all() and (LH.raw(_held(ctx)) == LH.raw(want[1])).all() and ctx._volume_dtype() == info
        for bad in (dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(max_radius=0.5), dict(max_radius=math.inf), dict(gain=0.0), dict(gain=-1.0)):
            with pytest.raises(ValueError):
                ctx.local_thickness(0.3, **bad)
        with pytest.raises(V.VokselisError) as e:
            ctx.local_thickness(0.3, max_radius=33.0)
        assert e.value.code == INVALID and "VK_THICK_MAX_REACH" in str(e.value)
    finally:
        ctx.close()


def _bonsai():
    import __graft_entry__ as g

    g.build_host()
    return os.path.join(LH.ROOT, "vokselis_amd", "_lib", "bonsai")


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_bonsai_thickness_writes_the_restatements_map_of_the_fixed_case(V, libs, tmp_path, kind):  # noqa: F811
    """bonsai --thickness 6 --save-raw on the fixed case: the saved file is the restatement's dense array, bit for bit, the totals are printed,
    and --histogram reads the installed map."""
    vol, _, _ = _fixed(kind)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [_bonsai(), "--raw-u16" if kind == "u16" else "--raw", str(src), "--dims", "40", "32", "24", "--iso", "0.5", "--thickness", "6", "--save-raw", str(dst), "--histogram", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = TH.restate(libs[0], vol, kind, 0.5, math.inf, (1, 1, 1), 6.0)
    line = "thickness: [0.5, inf] cap 6 spacing 1 1 1: 3586 foreground voxels, largest thickness 12, 3017 saturated voxels, gain %.9g" % float(np.float32(1.0) / np.float32(6.0))
    assert line in r.stdout.splitlines(), r.stdout[-800:]
    got = np.fromfile(dst, vol.dtype).reshape(vol.shape)
    assert TH.differences((None, got, None), (None, want[1], None)) == ""


def test_bonsai_thickness_takes_the_range_from_components_and_spacing_gain_and_fill_from_their_flags(V, libs, tmp_path):  # noqa: F811
    vol, _, _ = _fixed("u8")
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [_bonsai(), "--raw", str(src), "--dims", "40", "32", "24", "--components", "0.5", "inf", "--thickness", "32", "0.0625", "--morph-spacing", "1", "1", "2",
            "--label-fill", "0.25", "--save-raw", str(dst), "--histogram", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = TH.restate(libs[0], vol, "u8", 0.5, math.inf, (1, 1, 2), 32.0, 0.0625, 0.25)
    assert int(want[2][1]) == 82 and len(np.unique(want[0])) == 14
    got = np.fromfile(dst, np.uint8).reshape(vol.shape)
    assert TH.differences((None, got, None), (None, want[1], None)) == "" and int(got[0, 0, 0]) == 64
    assert "thickness: [0.5, inf] cap 32 spacing 1 1 2: 3586 foreground voxels, largest thickness %.6g, 0 saturated voxels, gain 0.0625" % (2.0 * math.sqrt(82)) in r.stdout, r.stdout[-800:]
