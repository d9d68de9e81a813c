"""The X_timing debug parameters of the dense-output passes (label, distance, split, filter, resample) on the MI355X.  tools/*_quick.py
and every per-phase figure in DESIGN.md rest on them: with vk_debug_set_param("X_timing", k) a call brackets its k-th phase with the
context's timer events and is otherwise the same call.  For every phase number a pass documents: the status is 0, every output is bit
for bit the untimed call's, and vk_timer_elapsed_ms gives a finite value >= 0.  A phase the request does not run leaves the timer
refusing.  Two volumes of 33 x 20 x 7 -- no extent a multiple of a wave, of the distance transpose's 32-tile or of the label tile: u8
PACKED, and f16 LINEAR for the two-byte branch of the dense output.  No tolerance anywhere: outputs are compared as bytes."""
import ctypes as C
import math

import numpy as np
import pytest

from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPE = (7, 20, 33)
LO = 0.5           # the foreground: stored value >= 0.5 of full scale
SPLIT_RADIUS = 2.0  # leaves two markers of the two touching balls (np_split_reference on this volume: 38 regions, 2 markers, 21 cut)
NO_BRACKET = "no completed timer bracket"


def _volume(kind):
    """Noise below the range, two ellipsoids inside it that touch, and a sprinkle of lone voxels: 37 components, one of them large."""
    rng = np.random.default_rng(29)
    v = rng.integers(0, 100, SHAPE).astype(np.uint8)
    z, y, x = np.indices(SHAPE)
    for cx in (9, 23):
        ball = ((x - cx) / 8.0) ** 2 + ((y - 10) / 8.0) ** 2 + ((z - 3) / 3.5) ** 2 <= 1.0
        v[ball] = rng.integers(160, 256, SHAPE).astype(np.uint8)[ball]
    v[rng.random(SHAPE) < 0.02] = 255
    return v if kind == "u8" else (v.astype(np.float32) / 255.0).astype(np.float16)


def _context(V, kind):  # noqa: F811
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, _volume(kind), layout=V.LAYOUT_PACKED if kind == "u8" else V.LAYOUT_LINEAR)
    except BaseException:
        ctx.close()
        raise
    return ctx


@pytest.fixture(scope="module", params=["u8", "f16"])
def held(V, request):  # noqa: F811
    """(context, dtype): one context per volume for every pass -- no timed call installs."""
    ctx = _context(V, request.param)
    yield ctx, np.uint8 if request.param == "u8" else np.float16
    ctx.close()


def _bytes(*outs):
    return tuple(o.tobytes() if isinstance(o, np.ndarray) else C.string_at(C.addressof(o), C.sizeof(o)) for o in outs)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _label(V, ctx, dtype, lo=LO, dense=True):  # noqa: F811
    from vokselis_amd.label import label_request

    N = V.native
    lab, out, table, res = np.full(SHAPE, 0xABABABAB, np.uint32), np.full(SHAPE, 0xAB, np.uint8).astype(dtype) if dense else None, (N.VkComponent * 64)(), N.VkLabelResult()
    rc = N.lib().vk_label_components(ctx.handle, C.byref(label_request(lo, keep="largest", count=1)), None, _ptr(lab), table, 64, _ptr(out), C.byref(res))
    return rc, _bytes(lab, table, res) + (_bytes(out) if dense else ()), res


def _distance(V, ctx, dtype, op):  # noqa: F811
    from vokselis_amd.distance import MORPH_OPS, distance_request

    N = V.native
    morph = op in MORPH_OPS
    d2, out, res = None if morph else np.full(SHAPE, 0xABABABAB, np.uint32), np.full(SHAPE, 0xAB, np.uint8).astype(dtype) if morph else None, N.VkDistanceResult()
    req = distance_request(LO, op=op, radius=1.5 if morph else 0.0)
    rc = N.lib().vk_distance_transform(ctx.handle, C.byref(req), None, _ptr(d2), _ptr(out), C.byref(res))
    return rc, _bytes(out if morph else d2, res), res


def _split(V, ctx, dtype):  # noqa: F811
    from vokselis_amd.split import split_request

    N = V.native
    lab, out, table, res = np.full(SHAPE, 0xABABABAB, np.uint32), np.full(SHAPE, 0xAB, np.uint8).astype(dtype), (N.VkComponent * 64)(), N.VkSplitResult()
    rc = N.lib().vk_split_components(ctx.handle, C.byref(split_request(LO, radius=SPLIT_RADIUS)), None, _ptr(lab), table, 64, _ptr(out), C.byref(res))
    return rc, _bytes(lab, table, out, res), res


def _filter(V, ctx, dtype):  # noqa: F811
    from vokselis_amd.filter import filter_request

    out = np.full(SHAPE, 0xAB, np.uint8).astype(dtype)
    w = np.array([0.25, 0.5, 0.25], np.float32)
    rc = V.native.lib().vk_volume_filter(ctx.handle, C.byref(filter_request((w, w, w), "convolve", install=False)), _ptr(out))
    return rc, _bytes(out), None


def _resample(V, ctx, dtype):  # noqa: F811
    from vokselis_amd.resample import resample_request

    N = V.native
    out, res = np.full((4, 10, 17), 0xAB, np.uint8).astype(dtype), N.VkResampleResult()
    rc = N.lib().vk_volume_resample(ctx.handle, C.byref(resample_request((17, 10, 4), "area", install=False, out=True)), None, _ptr(out), C.byref(res))
    return rc, _bytes(out, res), res


def _elapsed_refused(V, ctx):  # noqa: F811
    with pytest.raises(V.native.VokselisError) as e:
        ctx.timer_elapsed_ms()
    return NO_BRACKET in str(e.value)


def _phases(ctx, param, phases, call):
    """The untimed call once; then the identical call under every phase number: status, bytes, a finite time."""
    rc, want, res = call()
    assert rc == 0
    try:
        for k in phases:
            ctx.set_param(param, k)
            rc, got, _ = call()
            assert rc == 0, (param, k)
            assert got == want, (param, k)
            ms = ctx.timer_elapsed_ms()
            assert math.isfinite(ms) and ms >= 0.0, (param, k, ms)
    finally:
        ctx.set_param(param, 0)
    return res


def test_label_phases(V, held):  # noqa: F811
    ctx, dtype = held
    res = _phases(ctx, "label_timing", range(1, 8), lambda: _label(V, ctx, dtype))
    assert res.n_components == 37 and res.n_kept_components == 1


def test_distance_phases(V, held):  # noqa: F811
    ctx, dtype = held
    res = _phases(ctx, "dist_timing", range(1, 8), lambda: _distance(V, ctx, dtype, "close"))
    assert res.n_foreground == 1906 and res.n_added == 385  # (np_dist_reference on this volume)
    _phases(ctx, "dist_timing", (7,), lambda: _distance(V, ctx, dtype, "outside"))


def test_split_phases(V, held):  # noqa: F811
    ctx, dtype = held
    res = _phases(ctx, "split_timing", range(1, 8), lambda: _split(V, ctx, dtype))
    assert res.n_markers == 2 and res.n_regions == 38 and res.n_cut == 21


def test_filter_phase(V, held):  # noqa: F811
    ctx, dtype = held
    _phases(ctx, "filter_timing", (1,), lambda: _filter(V, ctx, dtype))


def test_resample_phase_in_both_area_forms(V, held):  # noqa: F811
    ctx, dtype = held
    try:
        for passes in (0, 1):
            ctx.set_param("resample_area_passes", passes)
            res = _phases(ctx, "resample_timing", (1,), lambda: _resample(V, ctx, dtype))
            assert tuple(res.dims) == (17, 10, 4)
    finally:
        ctx.set_param("resample_area_passes", 0)


def test_a_label_phase_that_does_not_run_leaves_the_timer_refusing(V):  # noqa: F811
    ctx = _context(V, "u8")
    try:
        ctx.set_param("label_timing", 7)  # the mask: neither dense_out nor install
        rc, _, res = _label(V, ctx, np.uint8, dense=False)
        assert rc == 0 and res.n_components == 37 and _elapsed_refused(V, ctx)
        ctx.set_param("label_timing", 5)  # the numbering: no foreground, no component
        rc, _, res = _label(V, ctx, np.uint8, lo=2.0)
        assert rc == 0 and res.n_components == 0 and _elapsed_refused(V, ctx)
        ctx.set_param("label_timing", 0)
    finally:
        ctx.close()


def test_a_distance_phase_that_does_not_run_leaves_the_timer_refusing(V):  # noqa: F811
    ctx = _context(V, "u8")
    try:
        ctx.set_param("dist_timing", 4)  # the second round's columns: a dilation has one round
        rc, _, res = _distance(V, ctx, np.uint8, "dilate")
        assert rc == 0 and res.n_added == 1532 and _elapsed_refused(V, ctx)
        ctx.set_param("dist_timing", 0)
    finally:
        ctx.close()
