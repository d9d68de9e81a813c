"""vk_steady_diffusion on the MI355X.  Every shared case (tests/diff_cases.py) on every layout its format
supports: c_out, dense_out and the result -- sweeps, delta and both fluxes among them -- bitwise equal to the C restatement; a subset
again with the grids capped at 1, 3 and 7 workgroups and with the sweeps staged in LDS; three cases whose convergence falls in the first,
a middle and the last round of a batch of the host's loop, which is the test of the device's "done" word; the state a call without
INSTALL must leave alone; every refusal with its status and text and the outputs untouched.  There is no tolerance anywhere: every
comparison is of integers or of stored bits."""
import ctypes as C
import math

import numpy as np
import pytest

import diff_cases as DFC
import diff_helpers as DH
import label_helpers as LH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64
BATCH = 4  # kDiffBatch: the rounds the host enqueues between two looks at the counts


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return DH.build_restatement(tmp_path_factory.mktemp("diff_fuzz_gpu"))


@pytest.fixture(scope="module")
def expected(lib):
    """The restatement's output of every case, computed once and left unchanged."""
    out = {}
    for c in DFC.cases():
        e = DH.restate_case(lib, c)
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


def _case(word, kind, **where):
    return next(c for c in DFC.cases() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))


def _run_cases(V, ctx, cases, expected, kind, layout, caps, lds=0):  # noqa: F811
    uploaded = None
    ctx.set_param("diff_lds", lds)
    for i, c in enumerate(cases):
        if c.vol_id != uploaded:
            LH.upload(V, ctx, c.vol, kind, layout)
            uploaded = c.vol_id
        ctx.set_param("diff_max_blocks", caps[i % len(caps)])
        if c.clip is not None:
            ctx.set_clip_box(*c.clip)
        rc, got = DH.run(V, ctx, c)
        if c.clip is not None:
            ctx.set_clip_box(None)
        assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
        assert DH.differences(got, expected[c.name]) == "", (c.name, layout, caps[i % len(caps)], lds)


# ---- 1. every case on every layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [(k, l) for k in ("u8", "u16", "f16") for l in LH.LAYOUTS[k]])
def test_every_case_is_bitwise_the_restatement(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in DFC.cases() if c.kind == kind]
    assert len(cases) > 30
    ctx = _ctx(V)
    try:
        _run_cases(V, ctx, cases, expected, kind, layout, (0,))
    finally:
        ctx.close()


def _subset(kind):
    return [c for c in DFC.cases() if c.kind == kind and (tuple(reversed(c.vol.shape)) in (DFC.BIG, (64, 32, 16), (1, 1, 70), (1, 1, 1), (12, 7, 3)) or "sealed" in c.name)]


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_a_subset_again_with_every_grid_capped_at_one_three_and_seven_workgroups(V, expected, kind, layout):  # noqa: F811
    cases = _subset(kind)
    assert len(cases) > 10 and {c.axis for c in cases} == {0, 1, 2}
    ctx = _ctx(V)
    try:
        _run_cases(V, ctx, cases, expected, kind, layout, (1, 3, 7))
        _run_cases(V, ctx, cases[::2], expected, kind, layout, (7, 1, 3))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED"), ("u16", "PACKED"), ("f16", "LINEAR")])
def test_the_sweeps_staged_in_lds_give_the_same_bits(V, expected, kind, layout):  # noqa: F811
    cases = _subset(kind) + [c for c in DFC.cases() if c.kind == kind and tuple(reversed(c.vol.shape)) in ((37, 21, 11), (35, 19, 17)) and c.max_sweeps <= DFC.CAP]
    ctx = _ctx(V)
    try:
        _run_cases(V, ctx, cases, expected, kind, layout, (0, 3), lds=1)
    finally:
        ctx.close()


# ---- 2. the "done" word ------------------------------------------------------------------------------------------------------------------
def test_convergence_in_the_first_a_middle_and_the_last_round_of_a_batch_stops_the_sweeps_there(V, expected):  # noqa: F811
    """The host enqueues BATCH blocks blind: the launches behind the converged block must leave the state, and the count of sweeps, alone."""
    N = V.native
    picks = {"first": _case("the full block", "u8"), "middle": _case("the fixed set", "u8", check_every=32), "last": _case("a constriction", "u8")}
    blocks = {k: int(expected[c.name][2][DH.R["sweeps"]]) // c.check_every for k, c in picks.items()}
    assert all(int(expected[c.name][2][DH.R["converged"]]) == 1 for c in picks.values())
    assert blocks["first"] % BATCH == 1 and blocks["middle"] % BATCH in (2, 3) and blocks["last"] % BATCH == 0, blocks
    ctx = _ctx(V)
    try:
        for where, c in picks.items():
            LH.upload(V, ctx, c.vol, "u8", "PACKED")
            ctx.set_param("diff_timing", 9)
            rc, got = DH.run(V, ctx, c)
            words = N.lib().vk_last_error(ctx.handle).decode().split()
            ctx.set_param("diff_timing", 0)
            assert rc == 0 and DH.differences(got, expected[c.name]) == "", (where, c.name)
            assert words[:2] == ["diffusion:", "blocks"] and int(words[2]) == blocks[where] and int(words[6]) == blocks[where] * c.check_every, words
            # the launches: whole batches were enqueued, so more than the blocks that ran wherever the batch was not full
            per_block = 2 * c.check_every + 2
            assert int(words[4]) == per_block * BATCH * ((blocks[where] + BATCH - 1) // BATCH), words
    finally:
        ctx.close()


def test_two_runs_give_identical_bytes_and_absent_outputs_change_nothing(V, expected):  # noqa: F811
    N = V.native
    c = _case("density 0.6", "u16")
    ctx = _ctx(V, c.vol, "u16", "LINEAR")
    try:
        runs = [DH.run(V, ctx, c) for _ in range(2)]
        assert runs[0][0] == 0 and runs[1][0] == 0 and runs[0][1][0].tobytes() == runs[1][1][0].tobytes() and DH.differences(runs[0][1], expected[c.name]) == ""
        req, _ = DH.request(c)
        res = N.VkDiffusionResult()
        assert N.lib().vk_steady_diffusion(ctx.handle, C.byref(req), None, None, None, C.byref(res)) == 0           # the result alone
        assert (DH.result_array(res) == expected[c.name][2]).all() and res.sweeps == DFC.CAP and res.converged == 0  # ended by max_sweeps
        arr = np.zeros(c.vol.shape, np.float32)
        assert N.lib().vk_steady_diffusion(ctx.handle, C.byref(req), None, arr.ctypes.data, None, None) == 0        # c_out alone
        assert (arr.view(np.uint32) == expected[c.name][0].view(np.uint32)).all()
        dense = np.zeros_like(np.ascontiguousarray(c.vol))
        assert N.lib().vk_steady_diffusion(ctx.handle, C.byref(req), None, None, dense.ctypes.data, None) == 0       # dense_out alone
        assert (dense == expected[c.name][1]).all() and int(dense.max()) > 0
    finally:
        ctx.close()


# ---- 3. no install -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_a_call_without_install_leaves_the_context_as_it_was(V, expected, layout):  # noqa: F811
    c = _case("density 0.9", "u8", box=None)
    ctx = _ctx(V, c.vol, "u8", layout, k=2)
    try:
        info, empty = _info(V, ctx), _empty_fraction(V, ctx)
        before = _frame(V, ctx)
        hist = ctx.volume_histogram(256, (0.0, 1.0))
        counters = ctx.step_counts()
        rc, got = DH.run(V, ctx, c)
        assert rc == 0 and DH.differences(got, expected[c.name]) == ""
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
        assert rc2 == INVALID and msg.startswith("vk_steady_diffusion: VK_DIFF_INSTALL") and "a frame is being recorded" in msg and "vk_frame_begin / vk_frame_end" in msg
        assert (refused[0].view(np.uint32) == 0xABABABAB).all() and (refused[1] == 0x5A).all() and (refused[2][:9] == 7).all()
        assert _same_frame(ctx.read_frame(fid), before)
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
    finally:
        ctx.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_and_text_and_leaves_everything_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 33)).astype(np.uint8)
    out = np.full(vol.shape, 0xAB, np.uint8)
    c = np.full(vol.shape, 0xABABABAB, np.uint32)
    res = DH.fresh_result(N)
    ints = DH.RESULT

    def raw(ctx, req, box=None, want_c=True, dense=True, result=True):
        out[...] = 0xAB
        c[...] = 0xABABABAB
        for k in ints:
            setattr(res, k, 9)
        res.delta = res.omega = res.gain = 9.0
        rc = N.lib().vk_steady_diffusion(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, c.ctypes.data if want_c else None,
                                         out.ctypes.data if dense else None, C.byref(res) if result else None)
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((out == 0xAB).all() and (c == 0xABABABAB).all() and all(getattr(res, k) == 9 for k in ints) and res.delta == res.omega == res.gain == 9.0)

    def good(spacing=(1, 1, 1), **kw):
        r = N.VkDiffusionRequest()
        r.lo, r.hi, r.axis, r.check_every, r.max_sweeps, r.delta_tol, r.flux_tol = 0.5, math.inf, 0, 4, 8, 1e-5, 1e-3
        r.spacing[0], r.spacing[1], r.spacing[2] = spacing
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        info, empty, frame = _info(V, ctx), _empty_fraction(V, ctx), _frame(V, ctx)
        refused = [(None, {}, "the request is NULL"), (good(lo=math.nan), {}, "NaN"), (good(hi=math.nan), {}, "NaN"), (good(lo=0.6, hi=0.5), {}, "lo > hi"),
                   (good(lo=math.inf, hi=-math.inf), {}, "lo > hi")]
        refused += [(good(axis=k), {}, "axis must be 0, 1 or 2") for k in (3, 4, 0xffffffff)]
        refused += [(good(flags=f), {}, "unknown flag") for f in (4, 8, 1 << 31, 7)]
        refused += [(good(spacing=s), {}, "a spacing outside 1 .. VK_DIST_MAX_SPACING") for s in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (65, 1, 1), (1, 1, 0xffffffff))]
        refused += [(good(omega=v), {}, "omega must be 0 (automatic) or lie inside (0, 2)") for v in (2.0, -0.5, 2.5, math.nan, math.inf, -math.inf)]
        refused += [(good(check_every=v), {}, "check_every outside 1 .. VK_DIFF_MAX_CHECK_EVERY") for v in (0, 1025, 0xffffffff)]
        refused += [(good(check_every=4, max_sweeps=3), {}, "max_sweeps < check_every"), (good(check_every=1, max_sweeps=0), {}, "max_sweeps < check_every")]
        refused += [(good(delta_tol=v), {}, "delta_tol or flux_tol is negative or not finite") for v in (-1e-9, math.nan, math.inf)]
        refused += [(good(flux_tol=v), {}, "delta_tol or flux_tol is negative or not finite") for v in (-1.0, math.nan, math.inf)]
        refused += [(good(gain=v), {}, "gain or fill_out is not finite") for v in (math.nan, math.inf, -math.inf)]
        refused += [(good(fill_out=v), {}, "gain or fill_out is not finite") for v in (math.nan, math.inf)]
        refused += [(good(), dict(want_c=False, dense=False, result=False), "the result would go nowhere")]
        refused += [(good(), dict(box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the box is inverted or leaves the volume"), (good(), dict(box=N.VkVoxelBox(0, 0, 0, 34, 20, 7)), "leaves the volume"),
                    (good(flags=N.DIFF_CLIP_BOX), dict(box=N.VkVoxelBox(0, 0, 0, 1, 1, 1)), "VK_DIFF_CLIP_BOX takes the box from the clip box: box must be NULL")]
        # the order: the first of the header's list that applies is the one reported
        refused += [(good(lo=math.nan, axis=5, flags=4), {}, "NaN"), (good(axis=5, flags=4, spacing=(0, 1, 1)), {}, "axis must be"), (good(flags=4, spacing=(0, 1, 1), omega=3.0), {}, "unknown flag"),
                    (good(spacing=(0, 1, 1), omega=3.0, check_every=0), {}, "a spacing outside"), (good(omega=3.0, check_every=0), {}, "omega must be"),
                    (good(check_every=2000, max_sweeps=1, delta_tol=-1.0), {}, "check_every outside"), (good(max_sweeps=1, delta_tol=-1.0, gain=math.nan), {}, "max_sweeps < check_every"),
                    (good(delta_tol=-1.0, gain=math.nan), {}, "delta_tol or flux_tol"), (good(fill_out=math.nan), dict(want_c=False, dense=False, result=False), "gain or fill_out"),
                    (good(), dict(want_c=False, dense=False, result=False, box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the result would go nowhere")]
        for req, kw, word in refused:
            rc, msg = raw(ctx, req, **kw)
            assert rc == INVALID and word in msg and msg.startswith("vk_steady_diffusion: ") and untouched(), (word, rc, msg)
            assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        # what is accepted: infinite bounds, lo == hi, the largest spacing, zero tolerances, omega near its ends, a negative gain, the clip flag without a clip box, an empty box
        assert raw(ctx, good(lo=-math.inf, hi=math.inf, spacing=(64, 64, 64), delta_tol=0.0, flux_tol=0.0, omega=1.9999, gain=-1.0))[0] == 0 and res.n_foreground == vol.size == res.n_box
        assert res.n_inlet == res.n_outlet == 7 * 20 and res.sweeps == 8 and res.gain == -1.0 and res.omega == np.float32(1.9999)   # (so close to 2 the first sweeps overshoot far outside [0, 1]: nothing is said about the field)
        assert raw(ctx, good(lo=0.5, hi=0.5, flags=N.DIFF_CLIP_BOX, omega=1e-30))[0] == 0
        assert raw(ctx, good(), box=N.VkVoxelBox(3, 3, 3, 3, 3, 3))[0] == 0 and (c == N.DIFF_OFF).all() and res.n_foreground == 0 and res.n_box == 0 and res.converged == 1 and res.sweeps == 4
        assert res.omega == np.float32(2.0 / (1.0 + 3.141592653589793)) and res.gain == 1.0 and not out.any()
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and _same_frame(_frame(V, ctx), frame)
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            for r in (good(), good(flags=N.DIFF_INSTALL)):
                rc, msg = raw(ctx, r)
                assert rc == UNSUPPORTED and msg.startswith("diffusion: ") and "needs a scalar LINEAR, PACKED or PACKED_PAIRS volume" in msg and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, good())
        assert rc == UNSUPPORTED and msg.startswith("diffusion: ") and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()
