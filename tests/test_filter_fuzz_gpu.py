"""vk_volume_filter on the MI355X.  Every shared case (tests/filter_cases.py) on every layout its format supports,
dense_out bitwise equal to the C restatement; VK_FILTER_INSTALL against a fresh context that uploaded the restatement's output; the
state a dense_out-only call must leave alone, also inside an open frame; an install between frames in flight; every refusal with its
status and the volume unchanged; vk_filter_gaussian; the Python wrappers; the C++ host's bonsai --median --smooth --save-raw."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_cases as FC
import filter_helpers as FH
import np_filter_reference as NF
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return FH.build_restatement(tmp_path_factory.mktemp("filter_fuzz_gpu"))


@pytest.fixture(scope="module")
def expected(lib):
    """The restatement's output of every case, computed once and left unchanged."""
    out = {}
    for c in FC.cases():
        e = FH.restate_case(lib, c)
        e.setflags(write=False)
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
            FH.upload(V, ctx, vol, kind, layout)
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


# ---- 1. every case on every layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [(k, l) for k in ("u8", "u16", "f16") for l in FH.LAYOUTS[k]])
def test_every_case_is_bitwise_the_restatement(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in FC.cases() if c.kind == kind]
    assert len(cases) > 30
    ctx = _ctx(V)
    try:
        uploaded = None
        for i, c in enumerate(cases):
            if c.vol_id != uploaded:
                FH.upload(V, ctx, c.vol, kind, layout)
                uploaded = c.vol_id
            ctx.set_param("filter_max_blocks", (0, 1, 3)[i % 3])  # the grid-stride loop over tiles on small volumes too
            rc, got = FH.filter_dense(V, ctx, FH.request(V, c), c.vol)
            assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
            assert FH.differences(got, expected[c.name]) == "", (c.name, layout)
    finally:
        ctx.close()


# ---- 2. install ----------------------------------------------------------------------------------------------------------------------
def _install_cases():
    pick = ("u8 (33, 9, 10) uniform (every dimension), Gaussian sigma 2 radius 6, the maximum radius on every axis", "u8 (70, 19, 18) uniform (every dimension), MEDIAN3",
            "u8 (37, 5, 1) uniform (every dimension), sharpen, negative weights")
    by_name = {c.name: c for c in FC.cases()}
    out = [by_name[n] for n in pick]
    out.append(next(c for c in FC.cases() if c.kind == "u16" and "uniform" in c.vol_id and "dyadic" in c.name))
    out.append(next(c for c in FC.cases() if c.kind == "f16" and "normal with NaN" in c.vol_id and c.op == "median3"))
    out.append(next(c for c in FC.cases() if c.kind == "f16" and "uniform" in c.vol_id and "Gaussian" in c.name))
    return out


@pytest.mark.parametrize("state", ["table", "isosurface"])
def test_install_is_a_fresh_upload_of_the_restatements_output(V, lib, expected, state):  # noqa: F811
    for c in _install_cases():
        for layout in FH.LAYOUTS[c.kind]:
            want = expected[c.name]
            twice = FH.restate(lib, want, c.kind, c.op, c.radii, c.weights)
            a, b = _ctx(V), _ctx(V)
            try:
                for ctx in (a, b):
                    if state == "table":
                        ctx.set_transfer_function(_table(V), (0.0, 1.0))
                    else:
                        ctx.set_isosurface(0.35, (0.9, 0.8, 0.7), 4)
                FH.upload(V, a, c.vol, c.kind, layout)
                FH.upload(V, b, want, c.kind, layout)
                before = _info(V, a)
                req = FH.request(V, c, install=True)
                assert V.native.lib().vk_volume_filter(a.handle, C.byref(req), None) == 0, V.native.lib().vk_last_error(a.handle)
                assert _info(V, a) == before == _info(V, b), (c.name, layout)
                assert _empty_fraction(V, a) == _empty_fraction(V, b), (c.name, layout)
                ha, hb = a.volume_histogram(256, (0.0, 1.0)), b.volume_histogram(256, (0.0, 1.0))
                assert (ha.counts == hb.counts).all() and (ha.n_nan, ha.n_below, ha.n_above, ha.n_finite) == (hb.n_nan, hb.n_below, hb.n_above, hb.n_finite)
                assert ha.stats.min == hb.stats.min and ha.stats.max == hb.stats.max
                assert _same_frame(_frame(V, a), _frame(V, b)), (c.name, layout, state)
                # the installed volume filtered again: the restatement applied twice (with dense_out and INSTALL together)
                rc, got = FH.filter_dense(V, a, req, c.vol)
                assert rc == 0 and FH.differences(got, twice) == "", (c.name, layout)
                rc, got = FH.filter_dense(V, a, FH.request(V, FC.cases()[0]._replace(op="convolve", weights=(None, None, None), radii=(0, 0, 0))), c.vol)
                assert rc == 0 and FH.differences(got, NF.canonical(twice)) == "", (c.name, layout)  # ... and it was installed
            finally:
                a.close()
                b.close()


# ---- 3. no install -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_a_dense_out_only_call_leaves_the_context_as_it_was(V, expected, layout):  # noqa: F811
    c = next(c for c in FC.cases() if c.name == "u8 (70, 19, 18) uniform (every dimension), Gaussian sigma 2 radius 6, the maximum radius on every axis")
    ctx = _ctx(V, c.vol, "u8", layout, k=2)
    try:
        ctx.set_transfer_function(_table(V), (0.0, 1.0))
        info, empty = _info(V, ctx), _empty_fraction(V, ctx)
        before = _frame(V, ctx)
        assert np.abs(before[..., :3]).sum() > 0
        hist = ctx.volume_histogram(256, (0.0, 1.0))
        rc, got = FH.filter_dense(V, ctx, FH.request(V, c), c.vol)
        assert rc == 0 and FH.differences(got, expected[c.name]) == ""
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        assert (ctx.volume_histogram(256, (0.0, 1.0)).counts == hist.counts).all()
        assert _same_frame(_frame(V, ctx), before)
        # inside an open frame: on the frame's stream, behind the render recorded there
        fid = ctx.frame_begin()
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
        rc, inside = FH.filter_dense(V, ctx, FH.request(V, c), c.vol)
        # an install is refused there, and changes nothing
        req = FH.request(V, c, install=True)
        rc2 = V.native.lib().vk_volume_filter(ctx.handle, C.byref(req), None)
        msg = V.native.lib().vk_last_error(ctx.handle).decode()
        ctx.frame_end()
        assert rc == 0 and FH.differences(inside, expected[c.name]) == ""
        assert rc2 == INVALID and "a frame is being recorded" in msg and "vk_frame_begin / vk_frame_end" in msg
        assert _same_frame(ctx.read_frame(fid), before)
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
    finally:
        ctx.close()


# ---- 4. frames in flight -------------------------------------------------------------------------------------------------------------
def test_an_install_between_frames_in_flight_drains(V, expected):  # noqa: F811
    c = next(c for c in FC.cases() if c.name == "u8 (70, 19, 18) uniform (every dimension), MEDIAN3")
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
            ctx.median_volume()
            for _ in range(3):
                ids.append(ctx.frame_begin())
                pipe.record(ctx)
                ctx.frame_end()
            frames[k] = [ctx.read_frame(i).copy() for i in ids[-min(k, 3):]]
        finally:
            ctx.close()
    for f in frames[3]:
        assert _same_frame(f, frames[1][-1])
    fresh = _ctx(V, expected[c.name], "u8", "PACKED")
    try:
        fresh.set_transfer_function(_table(V), (0.0, 1.0))
        assert _same_frame(_frame(V, fresh), frames[1][-1])
    finally:
        fresh.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_status_and_leaves_the_volume_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 33)).astype(np.uint8)
    out = np.full(vol.shape, 0xAB, np.uint8)

    def raw(ctx, req, dense=True):
        out[...] = 0xAB
        rc = N.lib().vk_volume_filter(ctx.handle, C.byref(req) if req is not None else None, out.ctypes.data if dense else None)
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((out == 0xAB).all())

    def good():
        r = N.VkVolumeFilter()
        r.radius[0] = 1
        r.weights[0][0], r.weights[0][1], r.weights[0][2] = 0.25, 0.5, 0.25
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        info, empty, frame = _info(V, ctx), _empty_fraction(V, ctx), _frame(V, ctx)
        refused = [(None, True, "NULL")]
        for op in (2, -1, 1 << 30):
            r = good(); r.op = op
            refused.append((r, True, "unknown op"))
        for flags in (2, 3, 4, 1 << 31):
            r = good(); r.flags = flags
            refused.append((r, True, "unknown flag"))
        for axis in range(3):
            for rad in (7, 1000, 0xffffffff):
                r = good(); r.radius[axis] = rad
                refused.append((r, True, "radius"))
        for bad in (float("nan"), float("inf"), -float("inf"), 1024.5, -2000.0):
            for axis, k in ((0, 0), (0, 2), (2, 4)):
                r = good(); r.radius[axis] = max(r.radius[axis], (k + 1) // 2); r.weights[axis][k] = bad
                refused.append((r, True, "weight"))
        refused.append((good(), False, "neither dense_out nor VK_FILTER_INSTALL"))
        for req, dense, word in refused:
            rc, msg = raw(ctx, req, dense)
            assert rc == INVALID and word in msg and msg.startswith("vk_volume_filter: ") and untouched(), (word, rc, msg)
            assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        # what is accepted: the bound itself, junk in the weights of a skipped axis and beyond 2 r, junk radii under the median
        r = good(); r.weights[0][0] = 1024.0; r.weights[0][2] = -1024.0; r.weights[1][0] = float("nan"); r.weights[0][3] = float("inf")
        assert raw(ctx, r)[0] == 0 and not untouched()
        r = good(); r.op = N.FILTER_MEDIAN3; r.radius[1] = 99; r.weights[2][1] = float("nan")
        assert raw(ctx, r)[0] == 0 and not untouched()
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and _same_frame(_frame(V, ctx), frame)
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            for r in (good(), N.VkVolumeFilter(N.FILTER_MEDIAN3, N.FILTER_INSTALL)):
                rc, msg = raw(ctx, r)
                assert rc == UNSUPPORTED and msg.startswith("filter: ") and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, good())
        assert rc == UNSUPPORTED and msg.startswith("filter: ") and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()


# ---- 6. vk_filter_gaussian ------------------------------------------------------------------------------------------------------------
def test_gaussian_weights_from_the_library_drive_the_kernel(V, lib):  # noqa: F811
    w = np.zeros(9, np.float32)
    assert V.native.lib().vk_filter_gaussian(1.25, 4, w.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert (w.view(np.uint32) == w[::-1].view(np.uint32)).all() and abs(float(w.astype(np.float64).sum()) - 1.0) <= 9 * 2.0 ** -24
    assert V.native.lib().vk_filter_gaussian(0.0, 4, w.ctypes.data_as(C.POINTER(C.c_float))) == INVALID
    vol = np.random.default_rng(9).integers(0, 65536, (10, 9, 33)).astype(np.uint16)
    ctx = _ctx(V, vol, "u16", "PACKED")
    try:
        from vokselis_amd.filter import filter_request

        rc, got = FH.filter_dense(V, ctx, filter_request((w, w, None), install=False), vol)
        assert rc == 0 and FH.differences(got, FH.restate(lib, vol, "u16", "convolve", (4, 4, 0), (w, w, None))) == ""
    finally:
        ctx.close()


# ---- 7. the Python wrappers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_python_wrappers_against_the_references(V, lib, kind, layout):  # noqa: F811
    rng = np.random.default_rng(12)
    vol = rng.uniform(-1.0, 2.0, (10, 9, 33)).astype(np.float16) if kind == "f16" else rng.integers(0, 256 if kind == "u8" else 65536, (10, 9, 33)).astype(NF.DTYPE[kind])
    ctx = _ctx(V, vol, kind, layout)
    try:
        info = _info(V, ctx)
        # smooth_volume: one sigma, out without install
        w = V.gaussian_weights(0.9)
        assert len(w) == 7
        got = ctx.smooth_volume(0.9, install=False, out=True)
        assert got.dtype == vol.dtype and FH.differences(got, FH.restate(lib, vol, kind, "convolve", (3, 3, 3), (w, w, w))) == ""
        assert FH.differences(got, NF.convolve(vol, kind, (3, 3, 3), (w, w, w))) == ""
        # per-axis sigmas, an axis skipped, an explicit radius
        w2 = V.gaussian_weights(2.0, 2)
        got = ctx.smooth_volume((2.0, None, 0.0), radius=2, install=False, out=True)
        assert FH.differences(got, FH.restate(lib, vol, kind, "convolve", (2, 0, 0), (w2, None, None))) == ""
        # filter_volume(out=True) with install: the output, and the volume behind it
        sharp = (FC.SHARPEN, None, FC.DYADIC)
        want = FH.restate(lib, vol, kind, "convolve", (1, 0, 1), sharp)
        got = ctx.filter_volume(sharp, out=True)
        assert FH.differences(got, want) == "" and _info(V, ctx) == info
        # median_volume on the installed volume
        got = ctx.median_volume(install=False, out=True)
        assert FH.differences(got, FH.restate(lib, want, kind, "median3", (0, 0, 0), None)) == ""
        assert FH.differences(got, NF.median3(want, kind)) == ""
        assert ctx.median_volume() is None and ctx.smooth_volume(1.0) is None
        with pytest.raises(V.VokselisError) as e:
            ctx.filter_volume((FC.DYADIC, None, None), install=False, out=False)
        assert e.value.code == INVALID
    finally:
        ctx.close()


# ---- 8. the C++ host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_bonsai_filters_before_anything_else_and_saves_the_filtered_volume(V, lib, tmp_path, kind):  # noqa: F811
    """bonsai --median --smooth SX SY SZ --save-raw: the file is the restatement's median, then its Gaussian (the library's weights), and
    --histogram counts that volume, not the loaded one."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(FH.ROOT, "vokselis_amd", "_lib", "bonsai")
    d = (33, 9, 10)
    rng = np.random.default_rng(31)
    vol = (rng.integers(0, 256, FC.shape(d)) * (1 if kind == "u8" else 257)).astype(NF.DTYPE[kind])
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [exe, "--raw-u16" if kind == "u16" else "--raw", str(src), "--dims"] + [str(v) for v in d] + ["--median", "--smooth", "0.8", "0", "1.2", "--save-raw", str(dst), "--histogram", "256"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    wx, wz = V.gaussian_weights(0.8), V.gaussian_weights(1.2)
    med = FH.restate(lib, vol, kind, "median3", (0, 0, 0), None)
    want = FH.restate(lib, med, kind, "convolve", (len(wx) // 2, 0, len(wz) // 2), (wx, None, wz))
    got = np.fromfile(dst, NF.DTYPE[kind]).reshape(vol.shape)
    assert FH.differences(got, want) == ""
    lines = r.stdout.splitlines()
    assert any(line.startswith("filter: median 3x3x3 gaussian sigma") for line in lines) and any(line.startswith("filtered volume: %d bytes" % want.nbytes) for line in lines)
    counts = {int(a): int(b) for a, b in (line.split() for line in lines if len(line.split()) == 2 and line.split()[0].isdigit())}
    ref = np.bincount(want.ravel().astype(np.int64) >> (0 if kind == "u8" else 8), minlength=256)
    assert counts == {i: int(n) for i, n in enumerate(ref) if n}
