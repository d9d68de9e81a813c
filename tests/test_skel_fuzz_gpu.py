"""vk_skeletonize on the MI355X.  Every shared case (tests/skel_cases.py) on every layout its format supports:
class_out, dense_out and the result bitwise equal to the C restatement, a subset again with the grids capped at 1, 3 and 7 workgroups so
that every grid-stride loop runs; the state a call without INSTALL must leave alone; every refusal with its status and text and the
outputs untouched.  There is no tolerance anywhere: every comparison is of integers or of stored bits."""
import ctypes as C
import math

import numpy as np
import pytest

import label_helpers as LH
import skel_cases as SC
import skel_helpers as SH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64
KIND = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("skel_fuzz_gpu"))


@pytest.fixture(scope="module")
def expected(lib):
    """The restatement's output of every case, computed once and left unchanged."""
    out = {}
    for c in SC.cases():
        e = SH.restate_case(lib, c)
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
    return next(c for c in SC.cases() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))


def _run_cases(V, ctx, cases, expected, kind, layout, caps):  # noqa: F811
    uploaded = None
    for i, c in enumerate(cases):
        if c.vol_id != uploaded:
            LH.upload(V, ctx, c.vol, kind, layout)
            uploaded = c.vol_id
        ctx.set_param("skel_max_blocks", caps[i % len(caps)])
        if c.clip is not None:
            ctx.set_clip_box(*c.clip)
        rc, got = SH.run(V, ctx, c)
        if c.clip is not None:
            ctx.set_clip_box(None)
        assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
        assert SH.differences(got, expected[c.name]) == "", (c.name, layout, caps[i % len(caps)])


# ---- 1. every case on every layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [(k, l) for k in ("u8", "u16", "f16") for l in LH.LAYOUTS[k]])
def test_every_case_is_bitwise_the_restatement(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in SC.cases() if c.kind == kind]
    assert len(cases) > 30
    ctx = _ctx(V)
    try:
        _run_cases(V, ctx, cases, expected, kind, layout, (0,))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_a_subset_again_with_every_grid_capped_at_one_three_and_seven_workgroups(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in SC.cases() if c.kind == kind and tuple(reversed(c.vol.shape)) in (SC.BIG, SC.SHAPES, SC.LINE, (64, 32, 16), (1, 1, 70), (1, 1, 1))]
    assert len(cases) > 15 and {c.mode for c in cases} == {SC.CURVE, SC.KERNEL}
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
        runs = [SH.run(V, ctx, c) for _ in range(2)]
        assert runs[0][0] == 0 and runs[1][0] == 0 and runs[0][1][0].tobytes() == runs[1][1][0].tobytes() and SH.differences(runs[0][1], expected[c.name]) == ""
        req, _ = SH.request(c)
        res = N.VkSkeletonResult()
        assert N.lib().vk_skeletonize(ctx.handle, C.byref(req), None, None, None, C.byref(res)) == 0             # the result alone
        assert (SH.result_array(res) == expected[c.name][2]).all() and res.n_skeleton > 0
        cls = np.zeros(c.vol.shape, np.uint8)
        assert N.lib().vk_skeletonize(ctx.handle, C.byref(req), None, cls.ctypes.data, None, None) == 0           # class_out alone
        assert (cls == expected[c.name][0]).all()
        dense = np.zeros_like(np.ascontiguousarray(c.vol))
        assert N.lib().vk_skeletonize(ctx.handle, C.byref(req), None, None, dense.ctypes.data, None) == 0         # dense_out alone
        assert (dense == expected[c.name][1]).all() and ((dense != 0) == (cls != 0)).all()
        # the timed phases and the debug counts change no output: eight launches per iteration, whole batches
        for k in (1, 2, 3, 4, 9):
            ctx.set_param("skel_timing", k)
            rc, again = SH.run(V, ctx, c)
            words = N.lib().vk_last_error(ctx.handle).decode().split()
            assert rc == 0 and SH.differences(again, expected[c.name]) == "", k
            if k < 9:
                assert ctx.timer_elapsed_ms() >= 0.0
        ctx.set_param("skel_timing", 0)
        assert words[:2] == ["skeleton:", "iterations"] and int(words[2]) == res.iterations and int(words[4]) % 8 == 0 and int(words[4]) >= 8 * (res.iterations + 1), words
        assert int(words[8]) == res.n_foreground - res.n_skeleton and int(words[6]) >= int(words[4]) // 8, words
    finally:
        ctx.close()


# ---- 2. no install -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_a_call_without_install_leaves_the_context_as_it_was(V, expected, layout):  # noqa: F811
    c = _case("density 0.9", "u8", box=None, max_iterations=0)
    ctx = _ctx(V, c.vol, "u8", layout, k=2)
    try:
        info, empty = _info(V, ctx), _empty_fraction(V, ctx)
        before = _frame(V, ctx)
        hist = ctx.volume_histogram(256, (0.0, 1.0))
        counters = ctx.step_counts()
        rc, got = SH.run(V, ctx, c)
        assert rc == 0 and SH.differences(got, expected[c.name]) == ""
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and ctx.step_counts() == counters
        assert (ctx.volume_histogram(256, (0.0, 1.0)).counts == hist.counts).all()
        assert _same_frame(_frame(V, ctx), before)
        # inside an open frame: on the frame's stream, behind the render recorded there
        fid = ctx.frame_begin()
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
        rc, inside = SH.run(V, ctx, c)
        rc2, refused = SH.run(V, ctx, c, install=True)  # an install is refused there, and changes nothing
        msg = V.native.lib().vk_last_error(ctx.handle).decode()
        ctx.frame_end()
        assert rc == 0 and SH.differences(inside, expected[c.name]) == ""
        assert rc2 == INVALID and msg.startswith("vk_skeletonize: VK_SKEL_INSTALL") and "a frame is being recorded" in msg and "vk_frame_begin / vk_frame_end" in msg
        assert (refused[0] == 0xAB).all() and (refused[1] == 0x5A).all() and (refused[2] == 7).all()
        assert _same_frame(ctx.read_frame(fid), before)
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
    finally:
        ctx.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_and_text_and_leaves_everything_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 33)).astype(np.uint8)
    out = np.full(vol.shape, 0xAB, np.uint8)
    cls = np.full(vol.shape, 0xCD, np.uint8)
    res = SH.fresh_result(N)

    def raw(ctx, req, box=None, want_classes=True, dense=True, result=True):
        out[...] = 0xAB
        cls[...] = 0xCD
        for k in SH.RESULT + ("iterations", "converged"):
            setattr(res, k, 9)
        for j in range(13):
            res.links[j] = 9
        rc = N.lib().vk_skeletonize(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, cls.ctypes.data if want_classes else None,
                                    out.ctypes.data if dense else None, C.byref(res) if result else None)
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((out == 0xAB).all() and (cls == 0xCD).all() and (SH.result_array(res) == 9).all())

    def good(**kw):
        r = N.VkSkeletonRequest()
        r.lo, r.hi = 0.5, math.inf
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        info, empty, frame = _info(V, ctx), _empty_fraction(V, ctx), _frame(V, ctx)
        refused = [(None, {}, "the request is NULL"), (good(lo=math.nan), {}, "lo or hi is NaN"), (good(hi=math.nan), {}, "lo or hi is NaN"), (good(lo=0.6, hi=0.5), {}, "lo > hi"),
                   (good(lo=math.inf, hi=-math.inf), {}, "lo > hi")]
        refused += [(good(mode=k), {}, "unknown mode (VK_SKEL_CURVE, VK_SKEL_KERNEL)") for k in (2, 3, 1 << 31)]
        refused += [(good(flags=f), {}, "unknown flag (VK_SKEL_CLIP_BOX, VK_SKEL_INSTALL, VK_SKEL_FILL_IN)") for f in (8, 16, 1 << 31, 15)]
        refused += [(good(pad=1), {}, "pad must be 0")]
        refused += [(good(fill_out=v), {}, "fill_out is not finite") for v in (math.nan, math.inf, -math.inf)]
        refused += [(good(flags=N.SKEL_FILL_IN, fill_in=v), {}, "fill_in is not finite under VK_SKEL_FILL_IN") for v in (math.nan, math.inf, -math.inf)]
        refused += [(good(), dict(want_classes=False, dense=False, result=False), "none of class_out, dense_out, VK_SKEL_INSTALL and result: the result would go nowhere")]
        refused += [(good(), dict(box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the box is inverted or leaves the volume"), (good(), dict(box=N.VkVoxelBox(0, 0, 0, 34, 20, 7)), "leaves the volume"),
                    (good(flags=N.SKEL_CLIP_BOX), dict(box=N.VkVoxelBox(0, 0, 0, 1, 1, 1)), "VK_SKEL_CLIP_BOX takes the box from the clip box: box must be NULL")]
        # the order: the first of the header's list that applies is the one reported
        refused += [(good(lo=math.nan, mode=5, flags=8), {}, "NaN"), (good(lo=1.0, hi=0.0, mode=5), {}, "lo > hi"), (good(mode=5, flags=8, pad=3), {}, "unknown mode"),
                    (good(flags=8, pad=3, fill_out=math.nan), {}, "unknown flag"), (good(pad=3, fill_out=math.nan), {}, "pad must be 0"),
                    (good(fill_out=math.nan, fill_in=math.nan, flags=N.SKEL_FILL_IN), {}, "fill_out is not finite"),
                    (good(fill_in=math.nan, flags=N.SKEL_FILL_IN), dict(want_classes=False, dense=False, result=False), "fill_in is not finite"),
                    (good(), dict(want_classes=False, dense=False, result=False, box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the result would go nowhere")]
        for req, kw, word in refused:
            rc, msg = raw(ctx, req, **kw)
            assert rc == INVALID and word in msg and msg.startswith("vk_skeletonize: ") and untouched(), (word, rc, msg)
            assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        # what is accepted: infinite bounds, lo == hi, a fill_in that is not finite without its flag, the clip flag without a clip box, an empty box, a cap of one iteration
        assert raw(ctx, good(lo=-math.inf, hi=math.inf, mode=N.SKEL_KERNEL))[0] == 0 and res.n_foreground == vol.size and res.n_skeleton == 1 == res.n_isolated and res.converged == 1
        assert int((cls != 0).sum()) == 1 and int((out != 0).sum()) <= 1
        assert raw(ctx, good(lo=0.5, hi=0.5, flags=N.SKEL_CLIP_BOX, fill_in=math.nan))[0] == 0
        assert raw(ctx, good(), box=N.VkVoxelBox(3, 3, 3, 3, 3, 3))[0] == 0 and not cls.any() and not out.any() and res.n_foreground == 0 == res.iterations and res.converged == 1
        assert raw(ctx, good(lo=-math.inf, hi=math.inf, max_iterations=1))[0] == 0 and res.iterations == 1 and res.converged == 0 and 0 < res.n_skeleton < vol.size
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and _same_frame(_frame(V, ctx), frame)
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            for r in (good(), good(flags=N.SKEL_INSTALL)):
                rc, msg = raw(ctx, r)
                assert rc == UNSUPPORTED and msg.startswith("skeleton: ") and "needs a scalar LINEAR, PACKED or PACKED_PAIRS volume" in msg and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, good())
        assert rc == UNSUPPORTED and msg.startswith("skeleton: ") and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()
