"""vk_measure_components on the MI355X beyond the case list: after split_components(install=True) on section 27's fixed
case the call finds the split regions; the call changes no context state -- volume, table, isosurface and clip box are in force afterwards
and a frame rendered after equals the one rendered before, bitwise --; it is accepted between frame_begin and frame_end; the Python
wrapper against the restatement from both label sources; the C++ host: bonsai --measure out.csv."""
import math
import os
import subprocess

import numpy as np
import pytest

import label_helpers as LH
import measure_cases as MC
import measure_helpers as MH
import split_cases as SC
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 64, 64


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("measure_gpu")
    return MH.build_restatement(d), LH.build_restatement(d)


def _ctx(V):  # noqa: F811
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    return V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)


def _table(V):  # noqa: F811
    return V.transfer_table([(0.0, 0.0, 0.0, 0.0, 0.0), (0.3, 0.1, 0.2, 0.9, 0.0), (0.5, 1.0, 0.5, 0.1, 0.4), (1.0, 1.0, 1.0, 1.0, 0.9)], 64)


def _frame(V, ctx):  # noqa: F811
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
    return ctx.read_backbuffer().copy()


def _fixed():
    return next(c for c in SC.cases() if "fixed" in c.name and c.radius == 6.0)


def test_after_a_split_install_the_call_measures_the_split_regions(V, libs):  # noqa: F811
    """Section 27's fixed case -- two balls of radius 8 that overlap, a wire and a speck -- split at radius 6: regions of 2063, 1979 and 7
    voxels.  The cut removes voxels from the later region's side, so the measured sizes are those of label_components on the cut volume,
    which the restatement over that volume's labels gives; the two large centroids lie on opposite sides of the cut's plane."""
    c = _fixed()
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, c.vol, "u8", "PACKED")
        ctx.update()
        r = ctx.split_components(0.5, radius=6.0, labels=True, out=True, install=True)
        assert sorted(int(s) for s in r.sizes) == [7, 1979, 2063] and r.n_cut > 0
        m = ctx.measure_components(0.5)
        assert m.n == m.n_regions == 3 and m.scale == 255 and m.n_foreground == 4049 - r.n_cut
        cut_labels, n, _ = MH.case_labels(libs[1], MC.Case("fixed, cut", "", r.dense, "u8", 0.5, math.inf, 6, None, None, None, 0))
        want, fg = MH.restate(libs[0], r.dense, "u8", cut_labels, n)
        assert n == 3 and fg == m.n_foreground and MH.differences(MH.table_array((V.VkRegion * 3).from_buffer_copy(m.records.tobytes()), 3), want) == ""
        # every measured region lies inside one split region, and the split's sizes are the measured ones plus the cut voxels of that region
        cut = (r.labels != 0) & (cut_labels == 0)
        for k in range(1, 4):
            inside = np.unique(r.labels[cut_labels == k])
            assert len(inside) == 1
            assert int(m.sizes[k - 1]) + int((cut & (r.labels == inside[0])).sum()) == int(r.sizes[inside[0] - 1])
        big = [int(i) - 1 for i in m.largest(2)]
        xs = sorted(float(m.centroid[k, 0]) for k in big)
        cut_x = np.nonzero(cut)[2]
        assert xs[0] < cut_x.min() <= cut_x.max() < xs[1]                       # opposite sides of the cut
        assert abs(xs[0] - 10.0) < 1.5 and abs(xs[1] - 22.0) < 2.5 and np.abs(m.centroid[big, 1] - 11.0).max() < 0.5 and np.abs(m.centroid[big, 2] - 10.0).max() < 0.5
        assert (m.mean[big] == 1.0).all() and (m.std[big] == 0.0).all()
        # the labels of the split fed back in: the split's own regions, cut voxels included
        own = ctx.measure_components(labels=r.labels)
        assert own.n == 3 and sorted(int(s) for s in own.sizes) == [7, 1979, 2063] and own.n_foreground == 4049
    finally:
        ctx.close()


STATES = {
    "table, clip box": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_clip_box((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))),
    "isosurface": lambda V, c: c.set_isosurface(0.35, (0.9, 0.8, 0.7), 4),
}


@pytest.mark.parametrize("state", sorted(STATES))
def test_the_call_changes_no_context_state(V, libs, state):  # noqa: F811
    slabs = next(k for k in MC.cases() if "regions that share faces" in k.name and k.kind == "u8")
    c = MC.Case("the slabs' volume, its own range", "", slabs.vol, "u8", 0.5, math.inf, 6, None, None, None, 0)
    want, fg = MH.restate_case(libs[0], libs[1], c)
    want_slabs, _ = MH.restate_case(libs[0], libs[1], slabs)
    ctx = _ctx(V)
    try:
        STATES[state](V, ctx)
        in_force = (ctx.isosurface, ctx.clip_box, ctx.projection)
        LH.upload(V, ctx, c.vol, "u8", "PACKED")
        ctx.update()
        before = _frame(V, ctx)
        assert np.abs(before[..., :3]).sum() > 0
        info = ctx._volume_dtype()
        rc, got, _ = MH.run(V, ctx, c)                 # the library labels the range
        assert rc == 0 and len(want) > 3 and MH.differences(got, want) == ""
        rc, got, _ = MH.run(V, ctx, slabs)             # the caller's labels
        assert rc == 0 and MH.differences(got, want_slabs) == ""
        after = _frame(V, ctx)
        assert (after.view(np.uint32) == before.view(np.uint32)).all() and ctx._volume_dtype() == info
        assert (ctx.isosurface, ctx.clip_box, ctx.projection) == in_force and (in_force[0] is not None or in_force[1] is not None)
        held = ctx.keep_components(-math.inf, math.inf, keep="all", install=False, out=True)[0]   # the volume itself, as a dense array
        assert (held == c.vol).all()
    finally:
        ctx.close()


def test_the_call_is_accepted_while_a_frame_is_being_recorded(V, libs):  # noqa: F811
    c = next(c for c in MC.cases() if "the clip box" in c.name and c.kind == "u16")
    want, fg = MH.restate_case(libs[0], libs[1], c)
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, c.vol, "u16", "LINEAR")
        ctx.update()
        ctx.frames_in_flight(2)
        ctx.set_transfer_function(_table(V), (0.0, 1.0))   # a render under a clip box needs a table
        ctx.set_clip_box(*c.clip)
        single = None
        for _ in range(2):
            fid = ctx.frame_begin()
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
            rc, got, res = MH.run(V, ctx, c)
            ctx.frame_end()
            frame = ctx.read_frame(fid)
            assert rc == 0 and MH.differences(got, want) == "" and int(res.n_foreground) == fg
            assert single is None or (frame.view(np.uint32) == single.view(np.uint32)).all()
            single = frame
    finally:
        ctx.close()


def test_python_wrapper_against_the_restatement(V, libs):  # noqa: F811
    c = next(c for c in MC.cases() if "extremes" in c.name and c.lo == -1.0)
    want, fg = MH.restate_case(libs[0], libs[1], c)
    labels, n, _ = MH.case_labels(libs[1], c)
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, c.vol, "f16", "PACKED")
        ctx.update()
        as_table = lambda m: MH.table_array((V.VkRegion * max(m.n, 1)).from_buffer_copy(m.records.tobytes() or bytes(192)), m.n)
        m = ctx.measure_components(c.lo, c.hi, connectivity=c.conn)
        assert m.n == n == m.n_regions and m.n_foreground == fg and m.scale == 1 << 24 and m.dims == (37, 21, 11) and MH.differences(as_table(m), want) == ""
        k = int(m.largest(1)[0]) - 1
        sel = labels == k + 1
        v = np.asarray(c.vol)[sel].astype(np.float64)
        assert abs(m.mean[k] - v.mean()) <= 1e-12 and abs(m.min[k] - v.min()) == 0.0 and abs(m.max[k] - v.max()) == 0.0
        signed = lambda h: int(h) - (1 << 64) if int(h) >> 63 else int(h)
        assert [int(s) for s in m.sum_q] == [(signed(h) << 64) + int(l) for h, l in zip(want[:, 20], want[:, 21])] and min(int(s) for s in m.sum_q) < 0
        fed = ctx.measure_components(labels=labels)                             # max_label: labels.max()
        assert fed.n == n and MH.differences(as_table(fed), want) == ""
        more = ctx.measure_components(labels=labels, max_label=n + 3)           # unused ids: empty records, NaN where a quotient has no meaning
        assert more.n == n + 3 and (more.sizes[n:] == 0).all() and np.isnan(more.centroid[n:]).all() and np.isnan(more.mean[n:]).all() and not more.touches_border[n:].any()
        boxed = ctx.measure_components(c.lo, c.hi, connectivity=c.conn, box=((3, 2, 1), (30, 18, 9)))
        assert 0 < boxed.n_foreground < fg and (boxed.boxes[:, :3] >= (3, 2, 1)).all() and (boxed.boxes[:, 3:] <= (30, 18, 9)).all()
        with pytest.raises(V.VokselisError) as e:
            ctx.measure_components(labels=labels, max_label=max(n - 1, 1))
        assert e.value.code == -1 and n > 1
        with pytest.raises(V.VokselisError):
            ctx.measure_components(0.5, connectivity=7)
        with pytest.raises(ValueError):
            ctx.measure_components()
        with pytest.raises(ValueError):
            ctx.measure_components(labels=labels[:, :, :5])
    finally:
        ctx.close()


def test_bonsai_measure_writes_one_line_per_region(V, libs, tmp_path):  # noqa: F811
    """bonsai --iso 0.5 --measure out.csv on the fixed case written as a raw file: the printed totals are the restatement's, the CSV has one
    line per region, its voxel counts sum to n_foreground, and its columns are the Python host's to the printed digits."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(LH.ROOT, "vokselis_amd", "_lib", "bonsai")
    c = next(c for c in MC.cases() if "section 27's fixed case" in c.name)
    want, fg = MH.restate_case(libs[0], libs[1], c)
    d = SC.FIXED_DIMS
    src, dst = tmp_path / "fixed.raw", tmp_path / "out.csv"
    np.ascontiguousarray(c.vol).tofile(src)
    args = [exe, "--raw", str(src), "--dims"] + [str(v) for v in d] + ["--iso", "0.5", "--size", "64x64", "--morph-spacing", "1", "1", "2", "--measure", str(dst), "--frames", "1"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    lines = r.stdout.splitlines()
    assert "measure: [0.5, inf] connectivity 6: %d regions, %d foreground voxels of %d, spacing 1 1 2" % (len(want), fg, c.vol.size) in lines, lines[:12]
    assert len([line for line in lines if line.startswith("region ")]) == len(want) == 2
    rows = dst.read_text().splitlines()
    from vokselis_amd.measure import Measurements

    assert rows[0] == Measurements.CSV_HEADER and len(rows) == 1 + len(want)
    cells = [row.split(",") for row in rows[1:]]
    assert sum(int(row[1]) for row in cells) == fg and [int(row[0]) for row in cells] == [1, 2]
    res = V.VkMeasureResult()
    res.n_regions, res.n_foreground, res.records_written, res.scale = len(want), fg, len(want), 255
    m = Measurements(MH.regions_from_table(want), len(want), res, d)
    sp = (1.0, 1.0, 2.0)
    for k, row in enumerate(cells):
        assert [int(v) for v in row[1:9]] == [int(v) for v in want[k, :8]] and [int(v) for v in row[22:25]] == [int(v) for v in want[k, 24:27]]
        ours = list(m.centroid[k]) + [m.volume(sp)[k], m.equivalent_diameter(sp)[k]] + list(m.principal_lengths(sp)[k]) + [m.mean[k], m.std[k], m.min[k], m.max[k]]
        theirs = [float(v) for v in row[9:21]]
        assert np.allclose(theirs, ours, rtol=1e-12, atol=1e-9), (k, theirs, ours)   # double against exact-then-rounded: a few ulps, and Jacobi against eigh
        assert abs(float(row[25]) - m.surface_area(sp)[k]) <= 1e-9 and int(row[26]) == int(m.touches_border[k])
