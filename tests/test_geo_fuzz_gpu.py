"""vk_geodesic_distance on the MI355X.  Every shared case (tests/geo_cases.py) on every layout its format
supports: g_out, dense_out and the result bitwise equal to the C restatement, a subset again with the grids capped at 1, 3 and 7
workgroups so that every grid-stride loop runs; the state a call without INSTALL must leave alone; every refusal with its status and text
and the outputs untouched.  There is no tolerance anywhere: every comparison is of integers or of stored bits."""
import ctypes as C
import math

import numpy as np
import pytest

import geo_cases as GC
import geo_helpers as GH
import label_helpers as LH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64
KIND = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return GH.build_restatement(tmp_path_factory.mktemp("geo_fuzz_gpu"))


@pytest.fixture(scope="module")
def expected(lib):
    """The restatement's output of every case, computed once and left unchanged."""
    out = {}
    for c in GC.cases():
        e = GH.restate_case(lib, c)
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


def _case(word, kind, **where):
    return next(c for c in GC.cases() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))


def _run_cases(V, ctx, cases, expected, kind, layout, caps):  # noqa: F811
    uploaded = None
    for i, c in enumerate(cases):
        if c.vol_id != uploaded:
            LH.upload(V, ctx, c.vol, kind, layout)
            uploaded = c.vol_id
        ctx.set_param("geo_max_blocks", caps[i % len(caps)])
        if c.clip is not None:
            ctx.set_clip_box(*c.clip)
        rc, got = GH.run(V, ctx, c)
        if c.clip is not None:
            ctx.set_clip_box(None)
        assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
        assert GH.differences(got, expected[c.name]) == "", (c.name, layout, caps[i % len(caps)])


# ---- 1. every case on every layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [(k, l) for k in ("u8", "u16", "f16") for l in LH.LAYOUTS[k]])
def test_every_case_is_bitwise_the_restatement(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in GC.cases() if c.kind == kind]
    assert len(cases) > 30
    ctx = _ctx(V)
    try:
        _run_cases(V, ctx, cases, expected, kind, layout, (0,))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_a_subset_again_with_every_grid_capped_at_one_three_and_seven_workgroups(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in GC.cases() if c.kind == kind and (tuple(reversed(c.vol.shape)) in (GC.BIG, (64, 32, 16), (1, 1, 70), (1, 1, 1), GC.SERPENTINE) or "shortcut" in c.name)]
    assert len(cases) > 10 and {c.conn for c in cases} == {6, 18, 26}
    ctx = _ctx(V)
    try:
        _run_cases(V, ctx, cases, expected, kind, layout, (1, 3, 7))
        _run_cases(V, ctx, cases[::2], expected, kind, layout, (7, 1, 3))
    finally:
        ctx.close()


def test_two_runs_give_identical_bytes_and_absent_outputs_change_nothing(V, expected):  # noqa: F811
    N = V.native
    c = _case("density 0.31", "u16")
    ctx = _ctx(V, c.vol, "u16", "LINEAR")
    try:
        runs = [GH.run(V, ctx, c) for _ in range(2)]
        assert runs[0][0] == 0 and runs[1][0] == 0 and runs[0][1][0].tobytes() == runs[1][1][0].tobytes() and GH.differences(runs[0][1], expected[c.name]) == ""
        req, _ = GH.request(c)
        res = N.VkGeodesicResult()
        assert N.lib().vk_geodesic_distance(ctx.handle, C.byref(req), None, None, None, C.byref(res)) == 0           # the result alone
        assert (GH.result_array(res) == expected[c.name][2]).all() and res.max_g > 0
        g = np.zeros(c.vol.shape, np.uint32)
        assert N.lib().vk_geodesic_distance(ctx.handle, C.byref(req), None, g.ctypes.data, None, None) == 0           # g_out alone
        assert (g == expected[c.name][0]).all()
        dense = np.zeros_like(np.ascontiguousarray(c.vol))
        assert N.lib().vk_geodesic_distance(ctx.handle, C.byref(req), None, None, dense.ctypes.data, None) == 0       # dense_out alone
        assert (dense == expected[c.name][1]).all() and int(dense.max()) == 65535                                     # the automatic gain: the farthest voxel stores full scale
        # the debug count of rounds changes no output; the set spans three tiles from its source face, so at least three rounds ran
        ctx.set_param("geo_timing", 9)
        rc, again = GH.run(V, ctx, c)
        words = N.lib().vk_last_error(ctx.handle).decode().split()
        ctx.set_param("geo_timing", 0)
        assert rc == 0 and GH.differences(again, expected[c.name]) == "" and words[:2] == ["geodesic:", "rounds"] and int(words[2]) >= 3 and int(words[6]) >= int(words[2]), words
    finally:
        ctx.close()


# ---- 2. no install -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_a_call_without_install_leaves_the_context_as_it_was(V, expected, layout):  # noqa: F811
    c = _case("density 0.9", "u8", box=None)
    ctx = _ctx(V, c.vol, "u8", layout, k=2)
    try:
        info, empty = _info(V, ctx), _empty_fraction(V, ctx)
        before = _frame(V, ctx)
        hist = ctx.volume_histogram(256, (0.0, 1.0))
        counters = ctx.step_counts()
        rc, got = GH.run(V, ctx, c)
        assert rc == 0 and GH.differences(got, expected[c.name]) == ""
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and ctx.step_counts() == counters
        assert (ctx.volume_histogram(256, (0.0, 1.0)).counts == hist.counts).all()
        assert _same_frame(_frame(V, ctx), before)
        # inside an open frame: on the frame's stream, behind the render recorded there
        fid = ctx.frame_begin()
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
        rc, inside = GH.run(V, ctx, c)
        rc2, refused = GH.run(V, ctx, c, install=True)  # an install is refused there, and changes nothing
        msg = V.native.lib().vk_last_error(ctx.handle).decode()
        ctx.frame_end()
        assert rc == 0 and GH.differences(inside, expected[c.name]) == ""
        assert rc2 == INVALID and msg.startswith("vk_geodesic_distance: VK_GEO_INSTALL") and "a frame is being recorded" in msg and "vk_frame_begin / vk_frame_end" in msg
        assert (refused[0] == 0xABABABAB).all() and (refused[1] == 0x5A).all() and (refused[2][:8] == 7).all()
        assert _same_frame(ctx.read_frame(fid), before)
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
    finally:
        ctx.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_and_text_and_leaves_everything_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 33)).astype(np.uint8)
    out = np.full(vol.shape, 0xAB, np.uint8)
    g = np.full(vol.shape, 0xABABABAB, np.uint32)
    res = GH.fresh_result(N)

    def raw(ctx, req, box=None, want_g=True, dense=True, result=True):
        out[...] = 0xAB
        g[...] = 0xABABABAB
        for k in GH.RESULT:
            setattr(res, k, 9)
        res.gain = 9.0
        rc = N.lib().vk_geodesic_distance(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, g.ctypes.data if want_g else None,
                                          out.ctypes.data if dense else None, C.byref(res) if result else None)
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((out == 0xAB).all() and (g == 0xABABABAB).all() and all(getattr(res, k) == 9 for k in GH.RESULT) and res.gain == 9.0)

    def good(spacing=(1, 1, 1), seeds=(), **kw):
        r = N.VkGeodesicRequest()
        r.lo, r.hi, r.connectivity, r.source_faces = 0.5, math.inf, 26, 1
        r.spacing[0], r.spacing[1], r.spacing[2] = spacing
        r.n_seeds = len(seeds)
        for k, s in enumerate(seeds):
            r.seeds[k][0], r.seeds[k][1], r.seeds[k][2] = s
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        info, empty, frame = _info(V, ctx), _empty_fraction(V, ctx), _frame(V, ctx)
        refused = [(None, {}, "the request is NULL"), (good(lo=math.nan), {}, "NaN"), (good(hi=math.nan), {}, "NaN"), (good(lo=0.6, hi=0.5), {}, "lo > hi"),
                   (good(lo=math.inf, hi=-math.inf), {}, "lo > hi")]
        refused += [(good(connectivity=k), {}, "connectivity must be 6, 18 or 26") for k in (0, 4, 8, 27)]
        refused += [(good(flags=f), {}, "unknown flag") for f in (4, 8, 1 << 31, 7)]
        refused += [(good(pad=1), {}, "pad must be 0")]
        refused += [(good(spacing=s), {}, "a spacing outside 1 .. VK_DIST_MAX_SPACING") for s in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65, 1, 1), (1, 1, 0xffffffff))]
        refused += [(good(source_faces=64), {}, "a face mask"), (good(target_faces=65), {}, "a face mask"), (good(source_faces=1 << 31), {}, "a face mask")]
        refused += [(good(n_seeds=17), {}, "n_seeds above VK_GEO_MAX_SEEDS"), (good(source_faces=0), {}, "no source")]
        refused += [(good(gain=v), {}, "gain is negative or not finite") for v in (math.nan, math.inf, -1.0, -1e-30)]
        refused += [(good(fill_out=v), {}, "fill_out or fill_unreached is not finite") for v in (math.nan, math.inf, -math.inf)]
        refused += [(good(fill_unreached=v), {}, "fill_out or fill_unreached is not finite") for v in (math.nan, -math.inf)]
        refused += [(good(), dict(want_g=False, dense=False, result=False), "the result would go nowhere")]
        refused += [(good(seeds=((33, 0, 0),)), {}, "a seed lies outside the volume"), (good(seeds=((0, 0, 0), (0, 20, 0))), {}, "a seed lies outside the volume"),
                    (good(seeds=((32, 19, 7),)), {}, "a seed lies outside the volume")]
        refused += [(good(), dict(box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the box is inverted or leaves the volume"), (good(), dict(box=N.VkVoxelBox(0, 0, 0, 34, 20, 7)), "leaves the volume"),
                    (good(flags=N.GEO_CLIP_BOX), dict(box=N.VkVoxelBox(0, 0, 0, 1, 1, 1)), "VK_GEO_CLIP_BOX takes the box from the clip box: box must be NULL")]
        # the order: the first of the header's list that applies is the one reported
        refused += [(good(lo=math.nan, connectivity=5, flags=4), {}, "NaN"), (good(connectivity=5, flags=4, pad=3), {}, "connectivity must be"), (good(flags=4, pad=3, spacing=(0, 1, 1)), {}, "unknown flag"),
                    (good(pad=3, spacing=(0, 1, 1), source_faces=64), {}, "pad must be 0"), (good(spacing=(0, 1, 1), source_faces=64, n_seeds=17), {}, "a spacing outside"),
                    (good(source_faces=64, n_seeds=17, gain=-1.0), {}, "a face mask"), (good(n_seeds=17, gain=-1.0, source_faces=0), {}, "n_seeds above"),
                    (good(source_faces=0, gain=-1.0, fill_out=math.nan), {}, "no source"), (good(gain=-1.0, fill_out=math.nan), {}, "gain is negative"),
                    (good(fill_unreached=math.nan), dict(want_g=False, dense=False, result=False), "fill_out or fill_unreached"),
                    (good(seeds=((99, 0, 0),)), dict(box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "a seed lies outside the volume")]
        for req, kw, word in refused:
            rc, msg = raw(ctx, req, **kw)
            assert rc == INVALID and word in msg and msg.startswith("vk_geodesic_distance: ") and untouched(), (word, rc, msg)
            assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        # what is accepted: infinite bounds, lo == hi, the largest spacing, every face at once, the clip flag without a clip box, an empty box, a seed on the last voxel
        assert raw(ctx, good(lo=-math.inf, hi=math.inf, spacing=(64, 64, 64), source_faces=63, target_faces=63))[0] == 0 and res.n_foreground == vol.size == res.n_reached
        assert res.target_min == 0 and res.n_target_reached == res.n_sources and int(g.max()) == res.max_g == 3 * 16384 and res.gain == np.float32(1.0) / np.float32(3 * 16384) and int(out.max()) == 255
        assert raw(ctx, good(lo=0.5, hi=0.5, flags=N.GEO_CLIP_BOX))[0] == 0
        assert raw(ctx, good(), box=N.VkVoxelBox(3, 3, 3, 3, 3, 3))[0] == 0 and (g == 0xFFFFFFFF).all() and res.n_foreground == 0 and res.max_g == 0 and res.gain == 0.0 and not out.any()
        assert res.target_min == 0xFFFFFFFF
        assert raw(ctx, good(lo=-math.inf, hi=math.inf, connectivity=6, source_faces=0, seeds=((32, 19, 6),)))[0] == 0 and res.n_sources == 1 and res.max_g == 256 * (32 + 19 + 6) and g[6, 19, 32] == 0
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and _same_frame(_frame(V, ctx), frame)
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            for r in (good(), good(flags=N.GEO_INSTALL)):
                rc, msg = raw(ctx, r)
                assert rc == UNSUPPORTED and msg.startswith("geodesic: ") and "needs a scalar LINEAR, PACKED or PACKED_PAIRS volume" in msg and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, good())
        assert rc == UNSUPPORTED and msg.startswith("geodesic: ") and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()
