"""vk_label_components on the MI355X.  Every shared case (tests/label_cases.py) on every layout its format supports:
labels, component table, totals and dense_out bitwise equal to the C restatement, with the grids capped so that the grid-stride loops run;
a truncated table is a prefix; VK_LABEL_INSTALL against a fresh context that uploaded the restatement's output; the state a call without
INSTALL must leave alone, also inside an open frame; an install between frames in flight; every refusal with its status and text and the
volume unchanged; two runs with identical bytes; the cleaned stand-in through the mesh extraction; pick -> voxel_of -> KEEP_SEEDS; the
Python wrappers; the C++ host's bonsai --components and its keep flags.  There is no tolerance anywhere: every comparison is of integers or of stored bits."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import label_cases as LC
import label_helpers as LH
import np_label_reference as NL
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return LH.build_restatement(tmp_path_factory.mktemp("label_fuzz_gpu"))


@pytest.fixture(scope="module")
def expected(lib):
    """The restatement's output of every case, computed once and left unchanged."""
    out = {}
    for c in LC.cases():
        e = LH.restate_case(lib, c)
        for a in e:
            a.setflags(write=False)
        out[c.name] = e
    return out


def _ctx(V, vol=None, kind=None, layout="PACKED", k=1):  # noqa: F811
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        if k > 1:
            ctx.frames_in_flight(k)
        if vol is not None:
            kind = kind or {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}[vol.dtype]
            LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
    except BaseException:
        ctx.close()
        raise
    return ctx


def _info(V, ctx):  # noqa: F811
    dims, fmt, layout = (C.c_uint32 * 3)(), C.c_int(), C.c_int()
    V.native.check(ctx.handle, V.native.lib().vk_volume_info(ctx.handle, dims, C.byref(fmt), C.byref(layout), None))
    return tuple(dims), fmt.value, layout.value


def _empty_fraction(V, ctx):  # noqa: F811
    f = C.c_double(-1.0)
    V.native.check(ctx.handle, V.native.lib().vk_volume_empty_fraction(ctx.handle, C.byref(f)))
    return f.value


def _frame(V, ctx):  # noqa: F811
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
    return ctx.read_backbuffer().copy()


def _same_frame(a, b):
    return bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _table(V):  # noqa: F811
    return V.transfer_table([(0.0, 0.0, 0.0, 0.0, 0.0), (0.3, 0.1, 0.2, 0.9, 0.0), (0.5, 1.0, 0.5, 0.1, 0.4), (1.0, 1.0, 1.0, 1.0, 0.9)], 64)


def _dense(V, ctx, vol):  # noqa: F811
    """The volume the context holds now, as a dense array: KEEP_ALL over every value with nothing to fill."""
    c = LC.Case("", "", vol, LH_KIND[vol.dtype], -math.inf, math.inf, 6, None, None, "all", 0, (), False, 0.0)
    rc, got = LH.run(V, ctx, c, labels=False)
    assert rc == 0
    return got[3]


LH_KIND = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}


def _case(word, kind, **where):
    return next(c for c in LC.cases() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))


# ---- 1. every case on every layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [(k, l) for k in ("u8", "u16", "f16") for l in LH.LAYOUTS[k]])
def test_every_case_is_bitwise_the_restatement(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in LC.cases() if c.kind == kind]
    assert len(cases) > 60
    ctx = _ctx(V)
    try:
        uploaded = None
        for i, c in enumerate(cases):
            if c.vol_id != uploaded:
                LH.upload(V, ctx, c.vol, kind, layout)
                uploaded = c.vol_id
            ctx.set_param("label_max_blocks", (0, 1, 3)[i % 3])  # the grid-stride loops over tiles and chunks on small volumes too
            if c.clip is not None:
                ctx.set_clip_box(*c.clip)
            rc, got = LH.run(V, ctx, c)
            if c.clip is not None:
                ctx.set_clip_box(None)
            assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
            assert LH.differences(got, expected[c.name]) == "", (c.name, layout)
    finally:
        ctx.close()


def test_a_truncated_table_is_a_bitwise_prefix_and_absent_outputs_change_nothing(V, expected):  # noqa: F811
    c = _case("percolation", "u8", conn=6, keep="all", lo=0.5)
    want = expected[c.name]
    n = int(want[2][0])
    ctx = _ctx(V, c.vol, "u8", "PACKED")
    try:
        for cap in (1, 7, n - 1, n, n + 5):
            rc, got = LH.run(V, ctx, c, cap=cap, dense=False, labels=(cap == 7))
            assert rc == 0 and len(got[1]) == min(cap, n) and (got[1] == want[1][:cap]).all() and (got[2] == want[2]).all(), cap
        N = V.native
        req, _ = LH.request(c)
        res = N.VkLabelResult()
        assert N.lib().vk_label_components(ctx.handle, C.byref(req), None, None, None, 0, None, C.byref(res)) == 0  # the totals alone
        assert [res.n_components, res.n_foreground, res.n_kept_components, res.n_kept_voxels] == [int(v) for v in want[2]]
        lab = np.zeros(c.vol.shape, np.uint32)
        assert N.lib().vk_label_components(ctx.handle, C.byref(req), None, lab.ctypes.data, None, 0, None, None) == 0       # the labels alone
        assert (lab == want[0]).all()
    finally:
        ctx.close()


def test_two_runs_of_the_percolation_case_give_identical_bytes(V):  # noqa: F811
    c = _case("percolation", "u16", conn=26, keep="all")
    ctx = _ctx(V, c.vol, "u16", "LINEAR")
    try:
        runs = [LH.run(V, ctx, c) for _ in range(2)]
        assert runs[0][0] == 0 and runs[1][0] == 0 and LH.differences(runs[0][1], runs[1][1]) == ""
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][1], runs[1][1]))
    finally:
        ctx.close()


# ---- 2. install ----------------------------------------------------------------------------------------------------------------------
def _install_cases():
    return [_case("percolation", "u8", keep="largest", count=1, invert=False), _case("uniform noise", "u8", keep="min_size", count=4, invert=True),
            _case("uniform noise", "u16", keep="seeds", invert=False), _case("NaN, inf", "f16", lo=-1.0, conn=26), _case("serpentine", "f16", keep="largest")]


@pytest.mark.parametrize("state", ["table", "isosurface"])
def test_install_is_a_fresh_upload_of_the_restatements_output(V, expected, state):  # noqa: F811
    for c in _install_cases():
        for layout in LH.LAYOUTS[c.kind]:
            want = expected[c.name][3]
            a, b = _ctx(V), _ctx(V)
            try:
                for ctx in (a, b):
                    if state == "table":
                        ctx.set_transfer_function(_table(V), (0.0, 1.0))
                    else:
                        ctx.set_isosurface(0.35, (0.9, 0.8, 0.7), 4)
                LH.upload(V, a, c.vol, c.kind, layout)
                LH.upload(V, b, want, c.kind, layout)
                before = _info(V, a)
                rc, got = LH.run(V, a, c, install=True)      # with every output and INSTALL together
                assert rc == 0, V.native.lib().vk_last_error(a.handle)
                assert LH.differences(got, expected[c.name]) == "", (c.name, layout)
                assert _info(V, a) == before == _info(V, b), (c.name, layout)
                assert _empty_fraction(V, a) == _empty_fraction(V, b), (c.name, layout)
                assert _same_frame(_frame(V, a), _frame(V, b)), (c.name, layout, state)
                assert LH.differences((None, None, None, _dense(V, a, c.vol)), (None, None, None, want)) == "", (c.name, layout)  # ... and it was installed
            finally:
                a.close()
                b.close()


# ---- 3. no install -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_a_call_without_install_leaves_the_context_as_it_was(V, expected, layout):  # noqa: F811
    c = _case("percolation", "u8", keep="largest", count=1, invert=False)
    ctx = _ctx(V, c.vol, "u8", layout, k=2)
    try:
        ctx.set_transfer_function(_table(V), (0.0, 1.0))
        info, empty = _info(V, ctx), _empty_fraction(V, ctx)
        before = _frame(V, ctx)
        assert np.abs(before[..., :3]).sum() > 0
        hist = ctx.volume_histogram(256, (0.0, 1.0))
        counters = ctx.step_counts()
        rc, got = LH.run(V, ctx, c)
        assert rc == 0 and LH.differences(got, expected[c.name]) == ""
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and ctx.step_counts() == counters
        assert (ctx.volume_histogram(256, (0.0, 1.0)).counts == hist.counts).all()
        assert _same_frame(_frame(V, ctx), before)
        # inside an open frame: on the frame's stream, behind the render recorded there
        fid = ctx.frame_begin()
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
        rc, inside = LH.run(V, ctx, c)
        rc2, _ = LH.run(V, ctx, c, install=True)  # an install is refused there, and changes nothing
        msg = V.native.lib().vk_last_error(ctx.handle).decode()
        ctx.frame_end()
        assert rc == 0 and LH.differences(inside, expected[c.name]) == ""
        assert rc2 == INVALID and "a frame is being recorded" in msg and "vk_frame_begin / vk_frame_end" in msg
        assert _same_frame(ctx.read_frame(fid), before)
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
    finally:
        ctx.close()


# ---- 4. frames in flight -------------------------------------------------------------------------------------------------------------
def test_an_install_between_frames_in_flight_drains(V, expected):  # noqa: F811
    c = _case("percolation", "u8", keep="largest", count=1, invert=False)
    frames = {}
    for k in (1, 3):
        ctx = _ctx(V, c.vol, "u8", "PACKED", k=k)
        try:
            ctx.set_transfer_function(_table(V), (0.0, 1.0))
            pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0)
            ids = []
            for _ in range(3):
                ids.append(ctx.frame_begin())
                pipe.record(ctx)
                ctx.frame_end()
            assert ctx.keep_components(c.lo, c.hi, keep="largest", count=1, fill=c.fill, connectivity=c.conn)[0] is None
            for _ in range(3):
                ids.append(ctx.frame_begin())
                pipe.record(ctx)
                ctx.frame_end()
            frames[k] = [ctx.read_frame(i).copy() for i in ids[-min(k, 3):]]
        finally:
            ctx.close()
    for f in frames[3]:
        assert _same_frame(f, frames[1][-1])
    fresh = _ctx(V, expected[c.name][3], "u8", "PACKED")
    try:
        fresh.set_transfer_function(_table(V), (0.0, 1.0))
        assert _same_frame(_frame(V, fresh), frames[1][-1])
    finally:
        fresh.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_and_text_and_leaves_everything_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 33)).astype(np.uint8)
    out = np.full(vol.shape, 0xAB, np.uint8)
    lab = np.full(vol.shape, 0xABABABAB, np.uint32)
    comps = (N.VkComponent * 4)()
    res = N.VkLabelResult(9, 9, 9, 9)

    def raw(ctx, req, box=None, labels=True, components=False, cap=4, dense=True, result=True):
        out[...] = 0xAB
        lab[...] = 0xABABABAB
        rc = N.lib().vk_label_components(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, lab.ctypes.data if labels else None,
                                         comps if components else None, cap, out.ctypes.data if dense else None, C.byref(res) if result else None)
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((out == 0xAB).all() and (lab == 0xABABABAB).all() and res.n_components == 9 and res.n_kept_voxels == 9)

    def good(**kw):
        r = N.VkLabelRequest()
        r.lo, r.hi, r.connectivity = 0.5, math.inf, 6
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def seeded(n, at=(0, 0, 0)):
        r = good(keep=N.LABEL_KEEP_SEEDS, n_seeds=n)
        for k in range(min(n, 16)):
            r.seeds[k][0], r.seeds[k][1], r.seeds[k][2] = at
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        info, empty, frame = _info(V, ctx), _empty_fraction(V, ctx), _frame(V, ctx)
        refused = [(None, {}, "the request is NULL"), (good(lo=math.nan), {}, "NaN"), (good(hi=math.nan), {}, "NaN"), (good(lo=0.6, hi=0.5), {}, "lo > hi"),
                   (good(lo=math.inf, hi=-math.inf), {}, "lo > hi")]
        refused += [(good(fill=f), {}, "fill is not finite") for f in (math.nan, math.inf, -math.inf)]
        refused += [(good(connectivity=k), {}, "connectivity must be 6, 18 or 26") for k in (0, 4, 8, 27, 0xffffffff)]
        refused += [(good(flags=f), {}, "unknown flag") for f in (8, 16, 1 << 31, 15)]
        refused += [(good(keep=k), {}, "unknown keep value") for k in (4, -1, 1 << 30)]
        refused += [(good(pad=1), {}, "pad must be 0")]
        refused += [(good(count=1), {}, "count does not fit"), (good(keep=N.LABEL_KEEP_LARGEST), {}, "count does not fit"), (good(keep=N.LABEL_KEEP_MIN_SIZE), {}, "count does not fit"),
                    (good(keep=N.LABEL_KEEP_SEEDS, n_seeds=1, count=1), {}, "count does not fit")]
        refused += [(good(n_seeds=1), {}, "n_seeds does not fit"), (seeded(0), {}, "n_seeds does not fit"), (seeded(17), {}, "n_seeds does not fit"),
                    (good(keep=N.LABEL_KEEP_LARGEST, count=1, n_seeds=1), {}, "n_seeds does not fit")]
        refused += [(seeded(1, at), {}, "a seed lies outside the volume") for at in ((33, 0, 0), (0, 20, 0), (0, 0, 7), (0xffffffff, 0, 0))]
        refused += [(good(), dict(components=True, cap=0), "cap_components == 0")]
        refused += [(good(), dict(labels=False, dense=False, result=False), "the result would go nowhere")]
        refused += [(good(), dict(box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the box is inverted or leaves the volume"), (good(), dict(box=N.VkVoxelBox(0, 0, 0, 34, 20, 7)), "leaves the volume"),
                    (good(flags=N.LABEL_CLIP_BOX), dict(box=N.VkVoxelBox(0, 0, 0, 1, 1, 1)), "VK_LABEL_CLIP_BOX takes the box from the clip box: box must be NULL")]
        for req, kw, word in refused:
            rc, msg = raw(ctx, req, **kw)
            assert rc == INVALID and word in msg and msg.startswith("vk_label_components: ") and untouched(), (word, rc, msg)
            assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        # what is accepted: infinite bounds, lo == hi, junk in the seeds beyond n_seeds, the clip flag without a clip box, an empty box
        r = seeded(2, (32, 19, 6)); r.seeds[5][0] = 0xffffffff; r.lo, r.hi = -math.inf, math.inf
        assert raw(ctx, r)[0] == 0 and not untouched() and res.n_components == 1 and res.n_kept_voxels == vol.size
        assert raw(ctx, good(lo=0.5, hi=0.5, flags=N.LABEL_CLIP_BOX))[0] == 0
        assert raw(ctx, good(), box=N.VkVoxelBox(3, 3, 3, 3, 3, 3))[0] == 0 and res.n_components == 0 and not lab.any()
        res.n_components = res.n_foreground = res.n_kept_components = res.n_kept_voxels = 9
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and _same_frame(_frame(V, ctx), frame)
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            for r in (good(), good(flags=N.LABEL_INSTALL)):
                rc, msg = raw(ctx, r)
                assert rc == UNSUPPORTED and msg.startswith("label: ") and "needs a scalar LINEAR, PACKED or PACKED_PAIRS volume" in msg and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, good())
        assert rc == UNSUPPORTED and msg.startswith("label: ") and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()


# ---- 6. the end-to-end story ----------------------------------------------------------------------------------------------------------
def test_the_largest_component_of_the_stand_in_meshes_inside_its_bounding_box(V, lib):  # noqa: F811
    """keep_components(keep="largest"), then extract_isosurface.  Exact: the mesh is bit for bit the mesh of a fresh context that uploaded
    the restatement's cleaned volume; every vertex lies within the kept component's bounding box grown by one voxel (a vertex sits on a
    lattice edge between an inside and an outside texel centre, and only the kept component is inside any more)."""
    from oracle import oracle as O

    n, iso = 48, 0.3
    vol = O.volume_standin_u8(n)
    labels, table, result, want = LH.restate(lib, vol, "u8", iso, math.inf, 6, keep="largest", count=1)
    assert int(result[0]) >= 1 and int(result[2]) == 1
    a, b = _ctx(V, vol, "u8", "PACKED"), _ctx(V, want, "u8", "PACKED")
    try:
        before = a.extract_isosurface(iso)
        dense, res = a.keep_components(iso, keep="largest", out=True)
        assert LH.differences((None, None, None, dense), (None, None, None, want)) == "" and [res.n_components, res.n_kept_components] == [int(result[0]), 1]
        comps = b.label_components(iso)
        assert comps.n == 1 and int(comps.sizes[0]) == int(result[3])
        tris, ref = a.extract_isosurface(iso), b.extract_isosurface(iso)
        assert len(tris) > 0 and tris.shape == ref.shape and (tris.view(np.uint32) == ref.view(np.uint32)).all()
        k = int(np.argmax(table[:, 0]))
        lo3, hi3 = table[k, 2:5].astype(np.float64), table[k, 5:8].astype(np.float64)
        pts = tris.reshape(-1, 3).astype(np.float64) * n - 0.5  # in voxel-centre coordinates, exactly
        assert (pts >= lo3 - 1.0).all() and (pts <= hi3 - 1.0 + 1.0).all()
        verts, faces = V.weld(tris)
        assert len(faces) == len(tris) and len(verts) < 3 * len(tris) and len(tris) <= len(before)  # the islands' triangles are gone
    finally:
        a.close()
        b.close()


def test_pick_then_voxel_of_then_keep_seeds_keeps_the_component_under_the_pixel(V, lib):  # noqa: F811
    """Two blocks of full value; the threshold 0.75 puts the crossing three quarters of the way from the last outside texel centre to the
    first inside one, that is inside the first foreground voxel: voxel_of(hit.pos) is a voxel of the block the ray meets."""
    n = 33
    vol = np.zeros((n, n, n), np.uint8)
    vol[12:21, 12:21, 12:21] = 255   # around the centre the camera looks at
    vol[2:6, 2:6, 25:30] = 255
    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        ctx.set_isosurface(0.75, (1.0, 1.0, 1.0), V.ISO_MAX_REFINE)
        hit = ctx.pick(W // 2, H // 2)
        assert hit is not None
        seed = V.voxel_of(hit.pos, (n, n, n))
        assert vol[seed[2], seed[1], seed[0]] == 255 and all(12 <= s < 21 for s in seed)
        dense, res = ctx.keep_components(0.75, keep="seeds", seeds=[seed], install=False, out=True)
        want = LH.restate(lib, vol, "u8", 0.75, math.inf, 6, keep="seeds", seeds=[seed])
        assert LH.differences((None, None, None, dense), (None, None, None, want[3])) == ""
        assert [res.n_components, res.n_foreground, res.n_kept_components, res.n_kept_voxels] == [2, 729 + 80, 1, 729]
        assert dense[12:21, 12:21, 12:21].min() == 255 and int((dense != 0).sum()) == 729
        removed, res = ctx.keep_components(0.75, keep="seeds", seeds=[seed], invert=True, install=False, out=True)   # "remove the table": the same seed, inverted
        assert int((removed != 0).sum()) == 80 and res.n_kept_voxels == 729
    finally:
        ctx.close()


# ---- 7. the Python wrappers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_python_wrappers_against_the_references(V, lib, kind, layout):  # noqa: F811
    vol = LC.noise((33, 9, 10), kind, 12)
    ctx = _ctx(V, vol, kind, layout)
    try:
        info = _info(V, ctx)
        labels, table, result, _ = LH.restate(lib, vol, kind, 0.6, math.inf, 18)
        comps = ctx.label_components(0.6, connectivity=18, labels=True)
        assert comps.n == len(table) and comps.n_foreground == int(result[1]) and comps.labels.dtype == np.uint32 and (comps.labels == labels).all()
        assert (comps.sizes == table[:, 0]).all() and (comps.first == table[:, 1]).all() and (comps.boxes == table[:, 2:]).all()
        assert (comps.labels == NL.label(vol, kind, 0.6, math.inf, 18, None)[0]).all()
        assert ctx.label_components(0.6, connectivity=18).labels is None
        box = ((2, 1, 0), (30, 9, 7))
        boxed = ctx.label_components(0.2, 0.7, connectivity=26, box=box, labels=True)
        assert (boxed.labels == LH.restate(lib, vol, kind, 0.2, 0.7, 26, box=box[0] + box[1])[0]).all()
        ctx.set_clip_box((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
        clipped = ctx.label_components(0.6, box="clip", labels=True)
        ctx.set_clip_box(None)
        assert (clipped.labels == LH.restate(lib, vol, kind, 0.6, math.inf, 6, box=LC.clip_voxel_box((0.0, 0.0, 0.0), (0.5, 1.0, 1.0), (33, 9, 10)))[0]).all()
        # keep_components: out without install, then install, and the volume behind it
        big = [int(i) for i in comps.largest(2)]
        want = LH.restate(lib, vol, kind, 0.6, math.inf, 18, keep="largest", count=2, fill=0.25)
        dense, res = ctx.keep_components(0.6, keep="largest", count=2, fill=0.25, connectivity=18, install=False, out=True)
        assert dense.dtype == vol.dtype and LH.differences((None, None, None, dense), (None, None, None, want[3])) == "" and res.n_kept_components == 2
        assert res.n_kept_voxels == int(comps.sizes[np.array(big) - 1].sum())
        dense, res = ctx.keep_components(0.6, keep="min_size", count=3, invert=True, fill=1.0, connectivity=18, out=True)
        want = LH.restate(lib, vol, kind, 0.6, math.inf, 18, keep="min_size", count=3, invert=True, fill=1.0)
        assert LH.differences((None, None, None, dense), (None, None, None, want[3])) == "" and _info(V, ctx) == info
        assert LH.differences((None, None, None, _dense(V, ctx, vol)), (None, None, None, want[3])) == ""
        assert ctx.keep_components(0.6, keep="all")[0] is None
        with pytest.raises(ValueError):
            ctx.keep_components(0.6, install=False, out=False)
        with pytest.raises(ValueError):
            ctx.keep_components(0.6, keep="largest", count=0)
        with pytest.raises(V.VokselisError) as e:
            ctx.keep_components(0.6, keep="all", connectivity=7)
        assert e.value.code == INVALID
    finally:
        ctx.close()


def test_label_components_with_more_components_than_the_first_table_holds(V):  # noqa: F811
    """The wrapper asks with room for 4096 components and once more when there are more: the 3-D checkerboard has one per foreground voxel."""
    vol = LC.checkerboard((48, 40, 33), "u8")
    ctx = _ctx(V, vol, "u8", "LINEAR")
    try:
        comps = ctx.label_components(0.5, labels=True)
        first = np.flatnonzero(vol.ravel())
        assert comps.n == len(first) == 31680 and comps.n_foreground == comps.n and (comps.sizes == 1).all() and (comps.first == first).all()
        assert (comps.labels.ravel()[first] == np.arange(1, comps.n + 1)).all() and (comps.boxes[:, 3:] == comps.boxes[:, :3] + 1).all()
    finally:
        ctx.close()


# ---- 8. the C++ host ------------------------------------------------------------------------------------------------------------------
def _bonsai():
    import __graft_entry__ as g

    g.build_host()
    return os.path.join(LH.ROOT, "vokselis_amd", "_lib", "bonsai")


def _stl_vertices(path):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw, "<u4", 1, 80)[0])
    rec = np.frombuffer(raw, np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]), n, 84)
    return np.ascontiguousarray(rec["v"])


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_bonsai_cleans_the_volume_before_the_mesh_and_saves_it(V, lib, tmp_path, kind):  # noqa: F811
    """bonsai --components LO HI CONN --remove-voxel --drop-islands --keep-largest --label-fill --save-raw --mesh: the printed totals and
    largest components are the restatement's of the loaded volume; the saved file is the restatement applied in bonsai's fixed order
    (remove, islands, largest); the STL's vertices are bit for bit the mesh of a context that uploaded that file's volume."""
    d = (48, 40, 33)
    vol = LC.percolation(d, kind, 6)
    labels, table, result, _ = LH.restate(lib, vol, kind, 0.5, math.inf, 6)
    order = np.lexsort((table[:, 1].astype(np.int64), -table[:, 0].astype(np.int64)))
    x, y, z = (int(v) for v in (table[order[0], 1] % d[0], table[order[0], 1] // d[0] % d[1], table[order[0], 1] // (d[0] * d[1])))  # a voxel of the largest component
    src, dst, stl = tmp_path / "in.raw", tmp_path / "out.raw", tmp_path / "out.stl"
    vol.tofile(src)
    args = [_bonsai(), "--raw-u16" if kind == "u16" else "--raw", str(src), "--dims"] + [str(v) for v in d] + ["--components", "0.5", "inf", "6", "--keep-largest", "2", "--drop-islands", "3",
            "--remove-voxel", str(x), str(y), str(z), "--label-fill", "0.25", "--save-raw", str(dst), "--mesh", str(stl), "--mesh-iso", "0.5"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    lines = r.stdout.splitlines()
    assert "components: [0.5, inf] connectivity 6: %d components, %d foreground voxels of %d" % (int(result[0]), int(result[1]), vol.size) in lines
    printed = [line for line in lines if line.startswith("component ")]
    assert printed == ["component %d: %d voxels, first %d, box %d %d %d .. %d %d %d" % ((k + 1,) + tuple(int(v) for v in table[k])) for k in order[:10]]
    v1 = LH.restate(lib, vol, kind, 0.5, math.inf, 6, keep="seeds", seeds=[(x, y, z)], invert=True, fill=0.25)
    v2 = LH.restate(lib, v1[3], kind, 0.5, math.inf, 6, keep="min_size", count=3, fill=0.25)
    v3 = LH.restate(lib, v2[3], kind, 0.5, math.inf, 6, keep="largest", count=2, fill=0.25)
    assert int(v1[2][2]) == 1 and int(v3[2][2]) == 2 and int(v3[2][3]) > 0
    for name, v in (("remove-voxel", v1), ("drop-islands", v2), ("keep-largest", v3)):
        assert "%s: %d of %d components selected, %d of %d foreground voxels" % (name, int(v[2][2]), int(v[2][0]), int(v[2][3]), int(v[2][1])) in lines, name
    got = np.fromfile(dst, LC.DTYPE[kind]).reshape(vol.shape)
    assert LH.differences((None, None, None, got), (None, None, None, v3[3])) == ""
    ctx = _ctx(V, v3[3], kind, "PACKED")
    try:
        want = ctx.extract_isosurface(0.5)
    finally:
        ctx.close()
    tris = _stl_vertices(stl)
    assert len(want) > 0 and tris.shape == want.shape and (tris.view(np.uint32) == want.view(np.uint32)).all()


def test_bonsai_keeps_the_component_under_a_voxel_and_under_a_pixel(V, lib, tmp_path):  # noqa: F811
    """--iso V alone gives the range [V, inf) at connectivity 6; --keep-voxel and --keep-pick seed one KEEP_SEEDS call, on the render path
    (frames follow) as on the --histogram path."""
    n = 33
    vol = np.zeros((n, n, n), np.uint8)
    vol[12:21, 12:21, 12:21] = 255   # around the centre the camera looks at
    vol[2:6, 2:6, 25:30] = 255
    vol[28:31, 28:31, 1:3] = 255
    src = tmp_path / "blocks.raw"
    vol.tofile(src)
    base = [_bonsai(), "--raw", str(src), "--dims", str(n), str(n), str(n), "--iso", "0.75", "--iso-refine", "16", "--size", "64x64"]
    for extra, kept, tail in ((["--keep-pick", "32", "32"], 729, ["--frames", "1"]), (["--keep-voxel", "26", "3", "4"], 80, ["--frames", "1"]),
                              (["--keep-pick", "32", "32", "--keep-voxel", "1", "29", "30", "--keep-pick", "0", "0"], 729 + 18, ["--histogram", "4"])):
        dst = tmp_path / ("kept%d.raw" % kept)
        r = subprocess.run(base + extra + ["--save-raw", str(dst)] + tail, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (extra, r.stdout[-500:], r.stderr[-500:])
        got = np.fromfile(dst, np.uint8).reshape(vol.shape)
        assert int((got != 0).sum()) == kept and ((got == 0) | (got == vol)).all(), extra
        assert "keep-voxel: %d of 3 components selected, %d of %d foreground voxels" % (1 if kept != 747 else 2, kept, 729 + 80 + 18) in r.stdout.splitlines()
        if "--keep-pick" in extra:
            assert got[12:21, 12:21, 12:21].min() == 255 and any(line.startswith("keep-pick (32, 32): voxel ") for line in r.stdout.splitlines())
        if kept == 747:
            assert "keep-pick (0, 0): miss" in r.stdout.splitlines() and "3 %d" % kept in r.stdout.splitlines()  # the histogram counts the cleaned volume
