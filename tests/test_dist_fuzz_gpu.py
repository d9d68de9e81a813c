"""vk_distance_transform on the MI355X.  Every shared case (tests/dist_cases.py) on every layout its format supports:
d2_out, dense_out and the result bitwise equal to the C restatement, a subset again with the grids capped at 1 and at 3 workgroups so
that every grid-stride loop runs; VK_DIST_INSTALL followed by vk_label_components and vk_volume_histogram, which see the new volume; the
state a call without INSTALL must leave alone; every refusal with its status and text and the outputs untouched; the Python wrappers;
the C++ host's bonsai --morph.  There is no tolerance anywhere: every comparison is of integers or of stored bits."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import dist_cases as DC
import dist_helpers as DH
import label_cases as LC
import label_helpers as LH
import np_dist_reference as ND
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64
KIND = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return DH.build_restatement(tmp_path_factory.mktemp("dist_fuzz_gpu"))


@pytest.fixture(scope="module")
def label_lib(tmp_path_factory):
    return LH.build_restatement(tmp_path_factory.mktemp("dist_fuzz_gpu_label"))


@pytest.fixture(scope="module")
def expected(lib):
    """The restatement's output of every case, computed once and left unchanged (None: refused for overflow)."""
    out = {}
    for c in DC.cases():
        e = DH.restate_case(lib, c)
        for a in e or ():
            if a is not None:
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
            LH.upload(V, ctx, vol, kind or KIND[vol.dtype], layout)
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


def _dense(V, ctx, vol):  # noqa: F811
    """The volume the context holds now, as a dense array: a dilation by 0 of every value, which changes nothing."""
    c = DC._make(KIND[vol.dtype], "", vol, "dilate", lo=-math.inf, hi=math.inf)
    rc, got = DH.run(V, ctx, c)
    assert rc == 0
    return got[1]


def _case(word, kind, **where):
    return next(c for c in DC.cases() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))


def _run_cases(V, ctx, cases, expected, kind, layout, caps):  # noqa: F811
    uploaded = None
    for i, c in enumerate(cases):
        if c.vol_id != uploaded:
            LH.upload(V, ctx, c.vol, kind, layout)
            uploaded = c.vol_id
        ctx.set_param("dist_max_blocks", caps[i % len(caps)])
        if c.clip is not None:
            ctx.set_clip_box(*c.clip)
        rc, got = DH.run(V, ctx, c)
        if c.clip is not None:
            ctx.set_clip_box(None)
        if c.refused:
            msg = V.native.lib().vk_last_error(ctx.handle).decode()
            assert expected[c.name] is None and rc == UNSUPPORTED and msg.startswith("distance: ") and "0xFFFFFFFE" in msg, (c.name, rc, msg)
            assert (got[0] == 0xABABABAB).all() and (got[2] == 7).all(), c.name
            continue
        assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
        assert DH.differences(got, expected[c.name]) == "", (c.name, layout, caps[i % len(caps)])


# ---- 1. every case on every layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [(k, l) for k in ("u8", "u16", "f16") for l in LH.LAYOUTS[k]])
def test_every_case_is_bitwise_the_restatement(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in DC.cases() if c.kind == kind]
    assert len(cases) > 100
    ctx = _ctx(V)
    try:
        _run_cases(V, ctx, cases, expected, kind, layout, (0,))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_a_subset_again_with_every_grid_capped_at_one_and_at_three_workgroups(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in DC.cases() if c.kind == kind and tuple(reversed(c.vol.shape)) in ((300, 3, 2), (2, 300, 3), (3, 2, 300), (48, 40, 33), (1, 1, 1))]
    assert len(cases) > 40 and {c.op for c in cases} == set(ND.OPS)
    ctx = _ctx(V)
    try:
        _run_cases(V, ctx, cases, expected, kind, layout, (1, 3))
        ctx.set_param("dist_x_plain", 1)   # the x pass without its transposes: the line function along rows
        _run_cases(V, ctx, cases[::3], expected, kind, layout, (3, 0, 1))
    finally:
        ctx.close()


def test_two_runs_give_identical_bytes_and_absent_outputs_change_nothing(V, expected):  # noqa: F811
    N = V.native
    c = _case("percolation at density 0.31", "u16", op="outside", spacing=(2, 2, 5))
    m = _case("percolation at density 0.31", "u16", op="close", spacing=(2, 2, 5))
    ctx = _ctx(V, c.vol, "u16", "LINEAR")
    try:
        runs = [DH.run(V, ctx, c) for _ in range(2)]
        assert runs[0][0] == 0 and runs[1][0] == 0 and runs[0][1][0].tobytes() == runs[1][1][0].tobytes() and DH.differences(runs[0][1], expected[c.name]) == ""
        req, _ = DH.request(c)
        res = N.VkDistanceResult()
        assert N.lib().vk_distance_transform(ctx.handle, C.byref(req), None, None, None, C.byref(res)) == 0           # the result alone
        assert (DH.result_array(res) == expected[c.name][2]).all() and res.max_d2 > 0
        d2 = np.zeros(c.vol.shape, np.uint32)
        assert N.lib().vk_distance_transform(ctx.handle, C.byref(req), None, d2.ctypes.data, None, None) == 0        # d2_out alone
        assert (d2 == expected[c.name][0]).all()
        req, _ = DH.request(m)
        assert N.lib().vk_distance_transform(ctx.handle, C.byref(req), None, None, None, C.byref(res)) == 0           # a morphology op's counts alone
        assert (DH.result_array(res) == expected[m.name][2]).all() and res.n_added > 0
    finally:
        ctx.close()


# ---- 2. install ----------------------------------------------------------------------------------------------------------------------
def _install_cases():
    return [_case("porous block", "u8", op="close", radius=1.5), _case("joined by a bridge", "u16", op="open", radius=1.5), _case("NaN, inf", "f16", op="close", lo=-1.0),
            _case("percolation at density 0.31", "u8", op="close", clip=None, box=(5, 3, 2, 30, 31, 20))]


def test_install_is_a_fresh_upload_of_the_restatements_output_and_later_passes_see_it(V, expected, label_lib):  # noqa: F811
    for c in _install_cases():
        for layout in LH.LAYOUTS[c.kind]:
            want = expected[c.name][1]
            a, b = _ctx(V), _ctx(V)
            try:
                for ctx in (a, b):
                    ctx.set_isosurface(0.35, (0.9, 0.8, 0.7), 4)
                LH.upload(V, a, c.vol, c.kind, layout)
                LH.upload(V, b, want, c.kind, layout)
                before = _info(V, a)
                rc, got = DH.run(V, a, c, install=True)      # with every output and INSTALL together
                assert rc == 0, V.native.lib().vk_last_error(a.handle)
                assert DH.differences(got, expected[c.name]) == "", (c.name, layout)
                assert _info(V, a) == before == _info(V, b), (c.name, layout)
                assert _empty_fraction(V, a) == _empty_fraction(V, b), (c.name, layout)
                assert _same_frame(_frame(V, a), _frame(V, b)), (c.name, layout)
                assert DH.differences((None, _dense(V, a, c.vol), None), (None, want, None)) == "", (c.name, layout)  # ... and it was installed
                # vk_label_components and vk_volume_histogram see the new volume
                lo, hi = (c.lo, c.hi) if c.kind != "f16" else (0.25, math.inf)
                labels, table, result, _ = LH.restate(label_lib, want, c.kind, lo, hi, 6)
                comps = a.label_components(lo, hi, labels=True)
                assert comps.n == int(result[0]) and comps.n_foreground == int(result[1]) and (comps.labels == labels).all(), (c.name, layout)
                assert (a.volume_histogram(64, (0.0, 1.0)).counts == b.volume_histogram(64, (0.0, 1.0)).counts).all(), (c.name, layout)
            finally:
                a.close()
                b.close()


def test_close_leaves_one_component_and_open_leaves_two_on_the_device(V, expected):  # noqa: F811
    for word, op, before, after in (("porous block", "close", 2, 1), ("joined by a bridge", "open", 1, 2)):
        c = _case(word, "u8", op=op, radius=1.5)
        ctx = _ctx(V, c.vol, "u8", "PACKED")
        try:
            assert ctx.label_components(c.lo).n == before
            res = ctx.morph_volume(c.lo, op=op, radius=1.5, fill_in=c.fill_in, fill_out=c.fill_out)
            assert (DH.result_array(res) == expected[c.name][2]).all()
            assert ctx.label_components(c.lo).n == after, word
        finally:
            ctx.close()


# ---- 3. no install -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_a_call_without_install_leaves_the_context_as_it_was(V, expected, layout):  # noqa: F811
    c = _case("percolation at density 0.31", "u8", op="close", clip=None, box=None)
    d = _case("percolation at density 0.31", "u8", op="inside", box=None)
    ctx = _ctx(V, c.vol, "u8", layout, k=2)
    try:
        info, empty = _info(V, ctx), _empty_fraction(V, ctx)
        before = _frame(V, ctx)
        hist = ctx.volume_histogram(256, (0.0, 1.0))
        counters = ctx.step_counts()
        for case in (c, d):
            rc, got = DH.run(V, ctx, case)
            assert rc == 0 and DH.differences(got, expected[case.name]) == ""
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and ctx.step_counts() == counters
        assert (ctx.volume_histogram(256, (0.0, 1.0)).counts == hist.counts).all()
        assert _same_frame(_frame(V, ctx), before)
        # inside an open frame: on the frame's stream, behind the render recorded there
        fid = ctx.frame_begin()
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
        rc, inside = DH.run(V, ctx, c)
        rc2, refused = DH.run(V, ctx, c, install=True)  # an install is refused there, and changes nothing
        msg = V.native.lib().vk_last_error(ctx.handle).decode()
        ctx.frame_end()
        assert rc == 0 and DH.differences(inside, expected[c.name]) == ""
        assert rc2 == INVALID and "a frame is being recorded" in msg and "vk_frame_begin / vk_frame_end" in msg and not refused[1].any() and (refused[2] == 7).all()
        assert _same_frame(ctx.read_frame(fid), before)
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
    finally:
        ctx.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_and_text_and_leaves_everything_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 33)).astype(np.uint8)
    out = np.full(vol.shape, 0xAB, np.uint8)
    d2 = np.full(vol.shape, 0xABABABAB, np.uint32)
    res = N.VkDistanceResult(9, 9, 9, 9, 9, 9)

    def raw(ctx, req, box=None, want_d2=None, dense=None, result=True):
        morph = req is not None and N.DIST_DILATE <= req.op <= N.DIST_OPEN
        want_d2 = (not morph) if want_d2 is None else want_d2
        dense = morph if dense is None else dense
        out[...] = 0xAB
        d2[...] = 0xABABABAB
        res.n_foreground = res.n_result = res.n_added = res.n_removed = 9
        res.max_d2 = res.pad = 9
        rc = N.lib().vk_distance_transform(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, d2.ctypes.data if want_d2 else None,
                                           out.ctypes.data if dense else None, C.byref(res) if result else None)
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((out == 0xAB).all() and (d2 == 0xABABABAB).all() and res.n_foreground == 9 and res.n_removed == 9 and res.max_d2 == 9)

    def good(spacing=(1, 1, 1), **kw):
        r = N.VkDistanceRequest()
        r.lo, r.hi, r.op = 0.5, math.inf, N.DIST_OUTSIDE
        r.spacing[0], r.spacing[1], r.spacing[2] = spacing
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        info, empty, frame = _info(V, ctx), _empty_fraction(V, ctx), _frame(V, ctx)
        refused = [(None, {}, "the request is NULL"), (good(lo=math.nan), {}, "NaN"), (good(hi=math.nan), {}, "NaN"), (good(lo=0.6, hi=0.5), {}, "lo > hi"),
                   (good(lo=math.inf, hi=-math.inf), {}, "lo > hi")]
        refused += [(good(op=k), {}, "unknown op") for k in (6, -1, 1 << 30)]
        refused += [(good(flags=f), {}, "unknown flag") for f in (4, 8, 1 << 31, 7)]
        refused += [(good(spacing=s), {}, "a spacing outside 1 .. VK_DIST_MAX_SPACING") for s in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65, 1, 1), (1, 1, 0xffffffff))]
        refused += [(good(op=N.DIST_CLOSE, radius=r), {}, "the radius is not finite, is negative or lies above VK_DIST_MAX_RADIUS") for r in (math.nan, math.inf, -1.0, -0.5, 65536.0)]
        refused += [(good(radius=1.0), {}, "a radius with a distance op"), (good(op=N.DIST_INSIDE, radius=0.5), {}, "a radius with a distance op")]
        refused += [(good(**{f: v}), {}, "a fill is not finite") for f in ("fill_in", "fill_out") for v in (math.nan, math.inf, -math.inf)]
        refused += [(good(op=op, radius=1.0), dict(want_d2=True), "d2_out with a morphology op") for op in (N.DIST_DILATE, N.DIST_ERODE, N.DIST_CLOSE, N.DIST_OPEN)]
        refused += [(good(), dict(dense=True), "dense_out or VK_DIST_INSTALL with a distance op"), (good(op=N.DIST_INSIDE, flags=N.DIST_INSTALL), {}, "dense_out or VK_DIST_INSTALL with a distance op")]
        refused += [(good(), dict(want_d2=False, result=False), "the result would go nowhere"), (good(op=N.DIST_OPEN), dict(dense=False, result=False), "the result would go nowhere")]
        refused += [(good(), dict(box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the box is inverted or leaves the volume"), (good(), dict(box=N.VkVoxelBox(0, 0, 0, 34, 20, 7)), "leaves the volume"),
                    (good(flags=N.DIST_CLIP_BOX), dict(box=N.VkVoxelBox(0, 0, 0, 1, 1, 1)), "VK_DIST_CLIP_BOX takes the box from the clip box: box must be NULL")]
        for req, kw, word in refused:
            rc, msg = raw(ctx, req, **kw)
            assert rc == INVALID and word in msg and msg.startswith("vk_distance_transform: ") and untouched(), (word, rc, msg)
            assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        # what is accepted: infinite bounds, lo == hi, the largest spacing and radius, the clip flag without a clip box, an empty box
        assert raw(ctx, good(lo=-math.inf, hi=math.inf, spacing=(64, 64, 64)))[0] == 0 and not d2.any() and res.n_foreground == vol.size and res.max_d2 == 0
        assert raw(ctx, good(lo=0.5, hi=0.5, flags=N.DIST_CLIP_BOX))[0] == 0
        assert raw(ctx, good(), box=N.VkVoxelBox(3, 3, 3, 3, 3, 3))[0] == 0 and (d2 == N.DIST_INF).all() and res.n_foreground == 0 and res.max_d2 == 0
        assert raw(ctx, good(op=N.DIST_DILATE, radius=65535.0, fill_in=1.0))[0] == 0 and (out[vol < 128] == 255).all() and res.n_result == vol.size
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and _same_frame(_frame(V, ctx), frame)
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            for r in (good(), good(op=N.DIST_CLOSE, radius=1.0, flags=N.DIST_INSTALL)):
                rc, msg = raw(ctx, r)
                assert rc == UNSUPPORTED and msg.startswith("distance: ") and "needs a scalar LINEAR, PACKED or PACKED_PAIRS volume" in msg and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, good())
        assert rc == UNSUPPORTED and msg.startswith("distance: ") and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, np.zeros((1, 1, 1100), np.uint8), "u8", "LINEAR")  # the overflow bound: (64 * 1099)^2
    try:
        rc, msg = raw(ctx, good(spacing=(64, 1, 1)))
        assert rc == UNSUPPORTED and msg.startswith("distance: ") and "0xFFFFFFFE" in msg and untouched()
        rc, msg = raw(ctx, good(spacing=(64, 1, 1), op=N.DIST_ERODE, radius=2.0))
        assert rc == UNSUPPORTED and msg.startswith("distance: ") and untouched()
        assert raw(ctx, good(spacing=(59, 64, 64)))[0] == 0    # 59 * 1099 = 64841 <= 65535
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()


# ---- 5. the Python wrappers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_python_wrappers_against_the_references(V, lib, kind, layout):  # noqa: F811
    vol = LC.noise((33, 9, 10), kind, 12)
    ctx = _ctx(V, vol, kind, layout)
    try:
        info = _info(V, ctx)
        d2 = ctx.distance_transform(0.6)
        assert d2.dtype == np.uint32 and d2.shape == vol.shape and (d2 == DH.restate(lib, vol, kind, 0.6, math.inf, "outside", (1, 1, 1), 0.0, 0.0, 0.0)[0]).all()
        assert (d2 == ND.brute(ND.NL.foreground(vol, kind, 0.6, math.inf, None), (1, 1, 1))).all()
        inside = ctx.distance_transform(0.2, 0.7, which="inside", spacing=(2, 2, 5))
        assert (inside == DH.restate(lib, vol, kind, 0.2, 0.7, "inside", (2, 2, 5), 0.0, 0.0, 0.0)[0]).all()
        box = ((2, 1, 0), (30, 9, 7))
        assert (ctx.distance_transform(0.6, box=box, spacing=(3, 1, 2)) == DH.restate(lib, vol, kind, 0.6, math.inf, "outside", (3, 1, 2), 0.0, 0.0, 0.0, box[0] + box[1])[0]).all()
        ctx.set_clip_box((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
        clipped = ctx.distance_transform(0.6, box="clip")
        ctx.set_clip_box(None)
        assert (clipped == DH.restate(lib, vol, kind, 0.6, math.inf, "outside", (1, 1, 1), 0.0, 0.0, 0.0, LC.clip_voxel_box((0.0, 0.0, 0.0), (0.5, 1.0, 1.0), (33, 9, 10)))[0]).all()
        # morph_volume: out without install, then install, and the volume behind it
        want = DH.restate(lib, vol, kind, 0.6, math.inf, "open", (1, 1, 1), 1.0, 1.0, 0.25)
        dense, res = ctx.morph_volume(0.6, op="open", radius=1.0, fill_out=0.25, install=False, out=True)
        assert dense.dtype == vol.dtype and DH.differences((None, dense, DH.result_array(res)), want) == "" and _info(V, ctx) == info
        assert DH.differences((None, _dense(V, ctx, vol), None), (None, np.ascontiguousarray(vol), None)) == ""  # not installed
        want = DH.restate(lib, vol, kind, 0.6, math.inf, "close", (2, 2, 5), 5.0, 0.9, 0.0)
        res = ctx.morph_volume(0.6, op="close", radius=5.0, spacing=(2, 2, 5), fill_in=0.9)
        assert (DH.result_array(res) == want[2]).all() and res.n_added > 0 and res.n_removed == 0 and _info(V, ctx) == info
        assert DH.differences((None, _dense(V, ctx, vol), None), (None, want[1], None)) == ""
        for bad in (dict(op="shrink"), dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(spacing=(1.5, 1, 1)), dict(radius=-1.0), dict(radius=math.inf)):
            with pytest.raises(ValueError):
                ctx.morph_volume(0.6, **bad)
        with pytest.raises(ValueError):
            ctx.distance_transform(0.6, which="close")
        with pytest.raises(V.VokselisError) as e:
            ctx.morph_volume(0.6, fill_in=math.inf)
        assert e.value.code == INVALID
    finally:
        ctx.close()


# ---- 6. the C++ host ------------------------------------------------------------------------------------------------------------------
def _bonsai():
    import __graft_entry__ as g

    g.build_host()
    return os.path.join(LH.ROOT, "vokselis_amd", "_lib", "bonsai")


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_bonsai_closes_the_gap_before_it_keeps_the_largest_component(V, lib, label_lib, tmp_path, kind):  # noqa: F811
    """bonsai --morph close 1.5 --components LO HI --keep-largest 1 --save-raw: without the closing the largest component is half the block;
    with it the saved file is the label restatement's keep-largest of the distance restatement's closing, bit for bit."""
    d = (37, 21, 11)
    vol = DC.mask_volume(DC.porous_block(d), kind)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [_bonsai(), "--raw-u16" if kind == "u16" else "--raw", str(src), "--dims"] + [str(v) for v in d] + ["--morph", "close", "1.5", "--morph-fill", "0.75", "0", "--components", "0.5", "inf",
            "--keep-largest", "1", "--save-raw", str(dst), "--histogram", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    closed = DH.restate(lib, vol, kind, 0.5, math.inf, "close", (1, 1, 1), 1.5, 0.75, 0.0)
    kept = LH.restate(label_lib, closed[1], kind, 0.5, math.inf, 6, keep="largest", count=1)
    assert int(kept[2][0]) == 1 and int(closed[2][2]) > 0
    assert "morph close 1.5: %d voxels in the range, %d afterwards (%d added, %d removed)" % tuple(int(v) for v in closed[2][:4]) in r.stdout.splitlines(), r.stdout[-800:]
    got = np.fromfile(dst, LC.DTYPE[kind]).reshape(vol.shape)
    assert LH.differences((None, None, None, got), (None, None, None, kept[3])) == ""
    assert int(LH.restate(label_lib, vol, kind, 0.5, math.inf, 6)[2][0]) == 2   # the gap did separate the block


def test_bonsai_opens_with_a_spacing_and_takes_the_range_from_iso(V, lib, tmp_path):  # noqa: F811
    d = (37, 21, 11)
    vol = DC.mask_volume(DC.bridged_blobs(d), "u8")
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [_bonsai(), "--raw", str(src), "--dims"] + [str(v) for v in d] + ["--iso", "0.5", "--morph", "open", "3", "--morph-spacing", "2", "2", "2", "--save-raw", str(dst), "--histogram", "4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = DH.restate(lib, vol, "u8", 0.5, math.inf, "open", (2, 2, 2), 3.0, 1.0, 0.0)
    assert int(want[2][3]) > 0
    got = np.fromfile(dst, np.uint8).reshape(vol.shape)
    assert DH.differences((None, got, None), (None, want[1], None)) == ""
