"""vk_geodesic_distance on the MI355X, in use: VK_GEO_INSTALL followed by the passes that read the map --
vk_volume_histogram gives the distribution of distances, exactly what the restatement's dense array predicts, and a table render of it
stays finite; an install leaves table, projection, isosurface, lighting and clip box in force; the Python wrapper with its derived
values and the path back to a source; the C++ host's bonsai --geodesic on the issue's fixed case."""
import math
import os
import subprocess

import numpy as np
import pytest

import dist_cases as DC
import geo_cases as GC
import geo_helpers as GH
import label_helpers as LH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID = -1
W, H = 64, 64
X0, X1 = 1, 2
G_INF = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return GH.build_restatement(tmp_path_factory.mktemp("geo_gpu"))


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
    return DC.mask_volume(GC.fixed_mask(), kind)


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED"), ("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_install_then_histogram_and_a_table_render_read_the_distance_map(V, lib, kind, layout):  # noqa: F811
    """The fixed case at connectivity 6: the installed map is the restatement's dense array bit for bit, its histogram is that of a fresh
    upload of that array, and the table march renders it to finite pixels."""
    vol = _fixed(kind)
    g, dense, result = GH.restate(lib, vol, kind, 0.5, math.inf, 6, (1, 1, 1), X0, X1, fill_unreached=0.0)
    assert [int(v) for v in result[:8]] == [206, 21, 206, 0, 21, 531968, 5888, 4352]
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
        info = ctx._volume_dtype()
        t = ctx.geodesic_distance(0.5, sources=("x-",), targets=("x+",), connectivity=6, install=True, out=True, g=True)
        assert (t.g == g).all() and (LH.raw(t.dense) == LH.raw(dense)).all() and (GH.result_array(t) == result).all()
        assert t.percolates and t.target_distance == 17.0 and t.tortuosity("x") == 17 / 11 and t.max_distance == 23.0 and t.n_unreached == 0 and ctx._volume_dtype() == info
        assert (LH.raw(_held(ctx)) == LH.raw(dense)).all()                                          # ... and it was installed
        fresh = _ctx(V)
        try:
            LH.upload(V, fresh, dense, kind, layout)
            fresh.update()
            want = np.asarray(fresh.volume_histogram(64, (0.0, 1.0)).counts)
        finally:
            fresh.close()
        counts = np.asarray(ctx.volume_histogram(64, (0.0, 1.0)).counts)
        assert (counts == want).all() and int(counts.sum()) == vol.size and int(counts[0]) >= vol.size - 206 + 21   # the sources and the voxels off the set store 0
        assert LH.raw(dense).max() == LH.raw(np.array([{"u8": 255, "u16": 65535, "f16": 1.0}[kind]], vol.dtype))[0]   # the farthest voxel stores full scale
        ctx.set_transfer_function(_table(V), (0.0, 1.0))
        frame = _frame(V, ctx)
        assert np.isfinite(frame).all() and np.abs(frame[..., :3]).sum() > 0
    finally:
        ctx.close()


STATES = {
    "table, lighting, clip box": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_lighting((0.3, 0.5, 0.8)), c.set_clip_box((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))),
    "table, max projection": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_projection("max")),
    "isosurface": lambda V, c: c.set_isosurface(0.35, (0.9, 0.8, 0.7), 4),
}


@pytest.mark.parametrize("state", sorted(STATES))
def test_an_install_leaves_table_projection_isosurface_lighting_and_clip_box_in_force(V, lib, state):  # noqa: F811
    """Context a installs the distance map under the state; context b gets the same state and a fresh upload of the restatement's map:
    the two render the same frame bit for bit, which they would not if the install had dropped any of the state."""
    c = next(c for c in GC.cases() if c.kind == "u8" and "density 0.9" in c.name and c.box is None)
    dense = GH.restate_case(lib, c)[1]
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
        t = a.geodesic_distance(c.lo, c.hi, sources=("x-",), targets=("x+",), connectivity=c.conn, spacing=c.spacing)   # install is the default
        assert t.percolates and t.n_saturated == 0 and t.dense is None and t.g is None
        assert (a.isosurface, a.clip_box, a.projection) == in_force == (b.isosurface, b.clip_box, b.projection)
        fa, fb = _frame(V, a), _frame(V, b)
        assert (fa.view(np.uint32) == fb.view(np.uint32)).all() and np.isfinite(fa).all() and np.abs(fa[..., :3]).sum() > 0
        assert not (fa.view(np.uint32) == before.view(np.uint32)).all()                             # the map is not the volume it came from
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
        want = GH.restate(lib, vol, kind, 0.3, math.inf, 26, (1, 1, 1), X0, 0)
        t = ctx.geodesic_distance(0.3, install=False, out=True, g=True)                             # the defaults: from x-, no target, 26 neighbours, spacing 1, automatic gain
        assert t.g.dtype == np.uint32 and t.dense.dtype == vol.dtype and GH.differences((t.g, t.dense, GH.result_array(t)), want) == ""
        assert t.gain == float(np.float32(1.0) / np.float32(t.max_g)) and not t.percolates and t.tortuosity("x") == math.inf and t.extent == d
        assert (LH.raw(_held(ctx)) == LH.raw(np.ascontiguousarray(vol))).all() and ctx._volume_dtype() == info   # not installed
        far = np.unravel_index(np.argmax(np.where(t.g == G_INF, 0, t.g)), t.g.shape)
        path = V.geodesic_path(t.g, (far[2], far[1], far[0]), (1, 1, 1), 26)
        assert path[-1][0] == 0 and t.g[path[-1][2], path[-1][1], path[-1][0]] == 0 and t.distance[far] == t.max_distance
        totals = ctx.geodesic_distance(0.3, install=False)
        assert totals.g is None and totals.dense is None and (GH.result_array(totals) == want[2]).all()
        box = ((2, 1, 0), (30, 9, 7))
        seeds = ((5, 4, 3), (0, 0, 0))
        want = GH.restate(lib, vol, kind, 0.2, 0.8, 18, (1, 2, 3), 16, 32 | 2, seeds, 1.0 / 4096.0, 0.25, 0.5, box[0] + box[1])
        t = ctx.geodesic_distance(0.2, 0.8, sources=("z-",), seeds=seeds, targets=("z+", "x+"), connectivity=18, spacing=(1, 2, 3), gain=1.0 / 4096.0, fill_out=0.25, fill_unreached=0.5, box=box,
                                  install=False, out=True, g=True)
        assert GH.differences((t.g, t.dense, GH.result_array(t)), want) == "" and t.gain == 1.0 / 4096.0 and t.extent == (28, 8, 7)
        clip = ((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
        ctx.set_clip_box(*clip)
        t = ctx.geodesic_distance(0.3, sources=("x+",), targets=("x-",), connectivity=6, box="clip", install=False, g=True)
        ctx.set_clip_box(None)
        cb = LC.clip_voxel_box(clip[0], clip[1], d)
        want = GH.restate(lib, vol, kind, 0.3, math.inf, 6, (1, 1, 1), X1, X0, box=cb)
        assert (t.g == want[0]).all() and (GH.result_array(t) == want[2]).all() and t.extent == (cb[3] - cb[0], cb[4] - cb[1], cb[5] - cb[2])
        want = GH.restate(lib, vol, kind, 0.3, math.inf, 6, (3, 1, 1), 4, 8, (), 1.0 / 8192.0)
        t = ctx.geodesic_distance(0.3, sources=("y-",), targets=("y+",), connectivity=6, spacing=(3, 1, 1), gain=1.0 / 8192.0)
        assert (GH.result_array(t) == want[2]).all() and (LH.raw(_held(ctx)) == LH.raw(want[1])).all() and ctx._volume_dtype() == info
        for bad in (dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(connectivity=7), dict(sources=("q",)), dict(gain=-1.0), dict(seeds=((1, 2),))):
            with pytest.raises(ValueError):
                ctx.geodesic_distance(0.3, **bad)
        with pytest.raises(V.VokselisError) as e:
            ctx.geodesic_distance(0.3, sources=(), install=False)
        assert e.value.code == INVALID and "no source" in str(e.value)
        with pytest.raises(V.VokselisError) as e:
            ctx.geodesic_distance(0.3, seeds=((33, 0, 0),), install=False)
        assert e.value.code == INVALID and "a seed lies outside the volume" in str(e.value)
    finally:
        ctx.close()


def _bonsai():
    import __graft_entry__ as g

    g.build_host()
    return os.path.join(LH.ROOT, "vokselis_amd", "_lib", "bonsai")


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_bonsai_geodesic_writes_the_restatements_map_of_the_fixed_case(V, lib, tmp_path, kind):  # noqa: F811
    """bonsai --geodesic x- x+ --save-raw on the fixed case: the saved file is the restatement's dense array, bit for bit, and the totals,
    the percolation, the target distance and the tortuosity are printed."""
    vol = _fixed(kind)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [_bonsai(), "--raw-u16" if kind == "u16" else "--raw", str(src), "--dims", "12", "7", "3", "--components", "0.5", "inf", "6", "--geodesic", "x-", "x+", "--save-raw", str(dst),
            "--histogram", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = GH.restate(lib, vol, kind, 0.5, math.inf, 6, (1, 1, 1), X0, X1)
    lines = r.stdout.splitlines()
    assert "geodesic: [0.5, inf] connectivity 6 spacing 1 1 1: 206 foreground voxels, 21 sources, 206 reached, 0 unreached, largest distance 23, mean distance %.6g" % (531968 / (256 * 206)) in lines, r.stdout[-800:]
    assert "geodesic: percolates yes, target distance 17, tortuosity %.6g along x" % (17 / 11) in lines, r.stdout[-800:]
    got = np.fromfile(dst, vol.dtype).reshape(vol.shape)
    assert GH.differences((None, got, None), (None, want[1], None)) == ""


def test_bonsai_geodesic_takes_seeds_spacing_and_fill_from_their_flags_and_steps_to_26_neighbours_by_default(V, lib, tmp_path):  # noqa: F811
    vol = DC.mask_volume(GC.pocket((37, 21, 11)), "u8")
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [_bonsai(), "--raw", str(src), "--dims", "37", "21", "11", "--iso", "0.5", "--geodesic-voxel", "3", "4", "5", "--geodesic-voxel", "18", "0", "0", "--geodesic", "y-", "x+",
            "--morph-spacing", "1", "2", "3", "--label-fill", "0.25", "--save-raw", str(dst), "--histogram", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = GH.restate(lib, vol, "u8", 0.5, math.inf, 26, (1, 2, 3), 4, X1, ((3, 4, 5), (18, 0, 0)), 0.0, 0.25, 0.25)
    got = np.fromfile(dst, np.uint8).reshape(vol.shape)
    assert GH.differences((None, got, None), (None, want[1], None)) == "" and int(got[0, 0, 18]) == 64   # the wall stores the fill; the seed on it contributes nothing
    n_fg, n_src, n_reached = (int(v) for v in want[2][:3])
    assert n_reached == n_fg and "geodesic: [0.5, inf] connectivity 26 spacing 1 2 3: %d foreground voxels, %d sources, %d reached, 0 unreached" % (n_fg, n_src, n_reached) in r.stdout, r.stdout[-800:]
    assert "geodesic: percolates yes, target distance" in r.stdout and "along x" in r.stdout
