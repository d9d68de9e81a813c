"""vk_volume_resample on the MI355X.  Every shared case (tests/resample_cases.py) on every layout its source format
has, dense_out bitwise equal to the C restatement, a part of them with the grid capped at 1 and 3 workgroups; AREA's three structures,
each chosen by name, on the ratios the unrolled kernels take and on others; vk_resample_output; VK_RESAMPLE_INSTALL against
a fresh context that uploaded the restatement's output; the layout an install lands on; the state a dense_out-only call must leave
alone, also inside an open frame; an install between frames in flight; every refusal with its status and text, the buffer and the
volume untouched; the Python wrappers against both references; the C++ host's bonsai --crop --downsample --to-u8 --save-raw."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_resample_reference as NR
import resample_cases as RC
import resample_helpers as RH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64
FMT = {"u8": 0, "f16": 1, "u16": 3}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return RH.build_restatement(tmp_path_factory.mktemp("resample_fuzz_gpu"))


@pytest.fixture(scope="module")
def expected(lib):
    """The restatement's output of every case, computed once and left unchanged."""
    out = {}
    for c in RC.runnable():
        e = RH.restate_case(lib, c)
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
            RH.upload(V, ctx, vol, kind, layout)
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


def _same_histogram(a, b):
    ha, hb = a.volume_histogram(256, (0.0, 1.0)), b.volume_histogram(256, (0.0, 1.0))
    return bool((ha.counts == hb.counts).all()) and (ha.n_nan, ha.n_below, ha.n_above, ha.n_finite) == (hb.n_nan, hb.n_below, hb.n_above, hb.n_finite)


def _table(V):  # noqa: F811
    return V.transfer_table([(0.0, 0.0, 0.0, 0.0, 0.0), (0.3, 0.1, 0.2, 0.9, 0.0), (0.5, 1.0, 0.5, 0.1, 0.4), (1.0, 1.0, 1.0, 1.0, 0.9)], 64)


def _run_case(V, ctx, c):  # noqa: F811
    if c.clip is not None:
        ctx.set_clip_box(*c.clip)
    try:
        req, vb = RH.request(V, c, install=False, out=True)
        return RH.resample_dense(V, ctx, req, vb, c.dims, c.out)
    finally:
        if c.clip is not None:
            ctx.set_clip_box(None)


# ---- 1. every case on every layout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [(k, l) for k in RC.KINDS for l in RH.LAYOUTS[k]])
def test_every_case_is_bitwise_the_restatement(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in RC.cases() if c.kind == kind]
    assert len(cases) > 80
    ctx = _ctx(V)
    try:
        uploaded = None
        for i, c in enumerate(cases):
            if c.vol_id != uploaded:
                RH.upload(V, ctx, c.vol, kind, layout)
                uploaded = c.vol_id
            ctx.set_param("resample_max_blocks", (0, 0, 1, 3)[i % 4])  # the loop over tiles on small volumes too
            rc, got, res = _run_case(V, ctx, c)
            msg = V.native.lib().vk_last_error(ctx.handle).decode()
            if c.refused is not None:
                assert rc == c.refused and msg.startswith("resample: ") and not RH.raw(got).any(), (c.name, rc, msg)
                continue
            assert rc == 0, (c.name, msg)
            assert RH.differences(got, expected[c.name]) == "", (c.name, layout)
            assert (tuple(res.dims), res.format, res.layout) == (c.dims, FMT[c.out], 0), c.name
            assert (res.box.x0, res.box.y0, res.box.z0, res.box.x1, res.box.y1, res.box.z1) == c.box, c.name
    finally:
        ctx.close()


# ---- 1b. AREA's three structures, each named ------------------------------------------------------------------------------------------
STRUCTURES = {"unrolled": (1, 0), "loops": (0, 0), "passes": (1, 1)}   # name: (resample_area_unroll, resample_area_passes)


@pytest.mark.parametrize("structure", sorted(STRUCTURES))
@pytest.mark.parametrize("kind, layout", [(k, l) for k in RC.KINDS for l in RH.LAYOUTS[k]])
def test_every_area_structure_is_bitwise_the_restatement(V, expected, kind, layout, structure):  # noqa: F811
    """The AREA cases of the kind -- among them the blocks of 2, 3 and 4, the only ratios the unrolled kernels take -- through one
    structure, chosen by name, with the grid uncapped and capped at 1 and 3 workgroups."""
    unroll, passes = STRUCTURES[structure]
    blocks = [c for c in RC.runnable() if c.kind == kind and "blocks of" in c.name]
    assert sorted(tuple(nb // n for nb, n in zip((c.box[3] - c.box[0], c.box[4] - c.box[1], c.box[5] - c.box[2]), c.dims)) for c in blocks) == [(2, 2, 2), (3, 3, 3), (4, 4, 4)]
    others = [c for c in RC.runnable() if c.kind == kind and c.mode == "area" and "blocks of" not in c.name][:12]   # other ratios, maps, boxes
    ctx = _ctx(V)
    try:
        ctx.set_param("resample_area_unroll", unroll)
        ctx.set_param("resample_area_passes", passes)
        uploaded = None
        for c in blocks + others:
            if c.vol_id != uploaded:
                RH.upload(V, ctx, c.vol, kind, layout)
                uploaded = c.vol_id
            for cap in (0, 1, 3):
                ctx.set_param("resample_max_blocks", cap)
                rc, got, _ = _run_case(V, ctx, c)
                assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
                assert RH.differences(got, expected[c.name]) == "", (c.name, layout, structure, cap)
    finally:
        ctx.close()


def test_the_output_of_a_call_is_known_before_it_runs(V):  # noqa: F811
    """vk_resample_output: the extents, format, layout and box of a call, nothing launched; its refusals are the call's."""
    N = V.native
    vol = RC.noise((37, 10, 9), "u8", 7)
    ctx = _ctx(V, vol, "u8", "PACKED_PAIRS")
    try:
        info = _info(V, ctx)
        ctx.set_clip_box((0.13, 0.0, 0.21), (0.81, 0.77, 1.0))
        cb = RC.clip_voxel_box((0.13, 0.0, 0.21), (0.81, 0.77, 1.0), (37, 10, 9))
        res = N.VkResampleResult()
        req = V.resample_request((0, 5, 0), "area", "u16", None, None, "clip", install=True)
        assert N.lib().vk_resample_output(ctx.handle, C.byref(req), None, C.byref(res)) == 0
        assert (tuple(res.dims), res.format, res.layout) == ((cb[3] - cb[0], 5, cb[5] - cb[2]), 3, V.LAYOUT_PACKED)
        assert (res.box.x0, res.box.y0, res.box.z0, res.box.x1, res.box.y1, res.box.z1) == cb
        req = V.resample_request((2, 5, 9), "area", install=False, out=True)    # 37 -> 2
        assert N.lib().vk_resample_output(ctx.handle, C.byref(req), None, C.byref(res)) == UNSUPPORTED
        assert N.lib().vk_last_error(ctx.handle).decode().startswith("resample: ")
        req.flags = 0   # neither dense_out nor INSTALL: no refusal here, the call itself refuses it
        req.dims[0] = 19
        assert N.lib().vk_resample_output(ctx.handle, C.byref(req), None, C.byref(res)) == 0 and tuple(res.dims) == (19, 5, 9) and res.layout == 0
        assert N.lib().vk_resample_output(ctx.handle, C.byref(req), None, None) == INVALID
        assert N.lib().vk_resample_output(ctx.handle, None, None, C.byref(res)) == INVALID
        assert _info(V, ctx) == info
    finally:
        ctx.close()


# ---- 2. install ----------------------------------------------------------------------------------------------------------------------
def _install_cases():
    by_name = {c.name: c for c in RC.runnable()}
    out = [by_name[n] for n in by_name if n.startswith("u8 noise (70, 37, 5), blocks of 2")]
    out.append(next(c for c in RC.runnable() if c.kind == "u16" and c.mode == "linear" and c.out == "u8" and c.window == (0.25, 0.75)))
    out.append(next(c for c in RC.runnable() if c.kind == "f16" and c.out == "f16" and c.window is None and "edges (70" in c.vol_id and "(identity)" not in c.name and min(c.dims) > 1))
    out.append(next(c for c in RC.runnable() if c.kind == "u8" and c.mode == "linear" and c.out == "u16" and c.window is None and c.dims == (130, 64, 7)))
    out.append(next(c for c in RC.runnable() if c.kind == "u8" and c.mode == "area" and c.out == "u8" and "ratio 16 box" in c.name))
    assert len(out) == 5
    return out


@pytest.mark.parametrize("state", ["table", "isosurface"])
def test_install_is_a_fresh_upload_of_the_restatements_output(V, expected, state):  # noqa: F811
    for c in _install_cases():
        for layout in RH.LAYOUTS[c.kind]:
            want = expected[c.name]
            a, b = _ctx(V), _ctx(V)
            try:
                for ctx in (a, b):
                    if state == "table":
                        ctx.set_transfer_function(_table(V), (0.0, 1.0))
                    else:
                        ctx.set_isosurface(0.35, (0.9, 0.8, 0.7), 4)
                RH.upload(V, a, c.vol, c.kind, layout)
                # AUTO: the source's layout, PACKED where that is PACKED_PAIRS and the output is not u8
                landed = "PACKED" if layout == "PACKED_PAIRS" and c.out != "u8" else layout
                RH.upload(V, b, want, c.out, landed)
                req, vb = RH.request(V, c, install=True, out=False)
                res = V.native.VkResampleResult()
                rc = V.native.lib().vk_volume_resample(a.handle, C.byref(req), C.byref(vb) if vb is not None else None, None, C.byref(res))
                assert rc == 0, (c.name, V.native.lib().vk_last_error(a.handle))
                assert _info(V, a) == _info(V, b) == (c.dims, FMT[c.out], getattr(V, "LAYOUT_" + landed)), (c.name, layout)
                assert (tuple(res.dims), res.format, res.layout) == _info(V, a)
                assert _empty_fraction(V, a) == _empty_fraction(V, b), (c.name, layout)
                assert _same_histogram(a, b), (c.name, layout)
                assert _same_frame(_frame(V, a), _frame(V, b)), (c.name, layout, state)
                top = 1.0 if c.out == "f16" else 0.5
                la, lb = a.label_components(0.2, top, connectivity=6, labels=True), b.label_components(0.2, top, connectivity=6, labels=True)
                assert la.n == lb.n and la.n_foreground == lb.n_foreground and (la.labels == lb.labels).all() and (la.sizes == lb.sizes).all(), (c.name, layout)
                # the installed volume through the identity: it is the restatement's output
                ident = V.resample_request(None, "nearest", None, None, None, None, install=False, out=True)
                rc, got, _ = RH.resample_dense(V, a, ident, None, c.dims, c.out)
                assert rc == 0 and RH.differences(got, want) == "", (c.name, layout)
            finally:
                a.close()
                b.close()


def test_the_layout_an_install_lands_on(V, lib):  # noqa: F811
    vol = RC.noise((37, 9, 10), "u16", 3)
    want = RH.restate(lib, vol, "u16", (0, 0, 0, 37, 9, 10), "area", (19, 5, 5), "u8", (0.1, 0.6))
    # u16 -> u8 into PACKED_PAIRS by name: the fast path opens to 16-bit data
    a, b = _ctx(V, vol, "u16", "LINEAR"), _ctx(V, want, "u8", "PACKED_PAIRS")
    try:
        res = a.resample_volume((19, 5, 5), mode="area", fmt="u8", window=(0.1, 0.6), layout=V.LAYOUT_PACKED_PAIRS)
        assert _info(V, a) == _info(V, b) == ((19, 5, 5), 0, V.LAYOUT_PACKED_PAIRS) and res.layout == V.LAYOUT_PACKED_PAIRS
        assert _empty_fraction(V, a) == _empty_fraction(V, b) and _same_histogram(a, b) and _same_frame(_frame(V, a), _frame(V, b))
    finally:
        a.close()
        b.close()
    # AUTO from a PACKED_PAIRS source to a u16 output lands on PACKED; PACKED_PAIRS by name is refused and the old volume stays
    v8 = RC.noise((37, 9, 10), "u8", 4)
    a = _ctx(V, v8, "u8", "PACKED_PAIRS")
    try:
        info = _info(V, a)
        with pytest.raises(V.VokselisError) as e:
            a.resample_volume((19, 5, 5), fmt="u16", layout=V.LAYOUT_PACKED_PAIRS)
        assert e.value.code == UNSUPPORTED and "resample: " in str(e.value) and "PACKED_PAIRS" in str(e.value) and _info(V, a) == info
        with pytest.raises(V.VokselisError) as e:
            a.resample_volume((19, 5, 5), fmt="u16", layout=V.LAYOUT_STAGED)
        assert e.value.code == UNSUPPORTED and _info(V, a) == info
        res = a.resample_volume((19, 5, 5), fmt="u16")
        assert _info(V, a) == ((19, 5, 5), 3, V.LAYOUT_PACKED) and res.layout == V.LAYOUT_PACKED and res.format == 3
        got, _ = a.resample_volume(mode="nearest", install=False, out=True)
        assert RH.differences(got, RH.restate(lib, v8, "u8", (0, 0, 0, 37, 9, 10), "linear", (19, 5, 5), "u16", None)) == ""
    finally:
        a.close()


# ---- 3. no install -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_a_dense_out_only_call_leaves_the_context_as_it_was(V, expected, layout):  # noqa: F811
    c = next(c for c in RC.runnable() if c.vol_id == "u8 noise (70, 37, 5)" and "blocks of 2" in c.name)
    ctx = _ctx(V, c.vol, "u8", layout, k=2)
    try:
        ctx.set_transfer_function(_table(V), (0.0, 1.0))
        info, empty = _info(V, ctx), _empty_fraction(V, ctx)
        before = _frame(V, ctx)
        assert np.abs(before[..., :3]).sum() > 0
        hist = ctx.volume_histogram(256, (0.0, 1.0))
        rc, got, _ = _run_case(V, ctx, c)
        assert rc == 0 and RH.differences(got, expected[c.name]) == ""
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        assert (ctx.volume_histogram(256, (0.0, 1.0)).counts == hist.counts).all()
        assert _same_frame(_frame(V, ctx), before)
        # inside an open frame: on the frame's stream, behind the render recorded there
        fid = ctx.frame_begin()
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
        rc, inside, _ = _run_case(V, ctx, c)
        # an install is refused there, and changes nothing
        req, vb = RH.request(V, c, install=True, out=False)
        rc2 = V.native.lib().vk_volume_resample(ctx.handle, C.byref(req), C.byref(vb), None, None)
        msg = V.native.lib().vk_last_error(ctx.handle).decode()
        ctx.frame_end()
        assert rc == 0 and RH.differences(inside, expected[c.name]) == ""
        assert rc2 == INVALID and msg.startswith("resample: ") and "a frame is being recorded" in msg and "vk_frame_begin / vk_frame_end" in msg
        assert _same_frame(ctx.read_frame(fid), before)
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
    finally:
        ctx.close()


# ---- 4. frames in flight -------------------------------------------------------------------------------------------------------------
def test_an_install_between_frames_in_flight_drains(V, expected):  # noqa: F811
    c = next(c for c in RC.runnable() if c.vol_id == "u8 noise (70, 37, 5)" and "blocks of 2" in c.name)
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
            ctx.resample_volume(c.dims, box=(c.box[:3], c.box[3:]), mode="area")
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
def test_every_refusal_returns_its_status_and_leaves_the_buffer_and_the_volume_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 40)).astype(np.uint8)  # (40, 20, 7)
    out = np.full(2 * vol.size, 0xAB, np.uint8)
    res = N.VkResampleResult()

    def raw(ctx, req, dense=True, box=None):
        out[...] = 0xAB
        C.memset(C.byref(res), 0x5A, C.sizeof(res))
        rc = N.lib().vk_volume_resample(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, out.ctypes.data if dense else None, C.byref(res))
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((out == 0xAB).all()) and bytes(res) == b"\x5a" * C.sizeof(res)

    def good(**kw):
        r = N.VkResampleRequest(N.RESAMPLE_LINEAR, 0, (C.c_uint32 * 3)(20, 10, 7), N.RESAMPLE_KEEP_FORMAT, 0, 0.0, 0.0)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        info, empty, frame = _info(V, ctx), _empty_fraction(V, ctx), _frame(V, ctx)
        refused = [(None, True, None, INVALID, "NULL")]
        refused += [(good(mode=m), True, None, INVALID, "unknown mode") for m in (3, -1, 1 << 30)]
        refused += [(good(flags=f), True, None, INVALID, "unknown flag") for f in (8, 16 | 1, 1 << 31)]
        refused += [(good(format=f), True, None, INVALID, "unknown format") for f in (4, -2, 1 << 20)]
        refused.append((good(format=N.FMT_RGBA16F_PAIR), True, None, INVALID, "RGBA16F_PAIR"))
        for axis in range(3):
            r = good()
            r.dims[axis] = 65536
            refused.append((r, True, None, INVALID, "above 65535"))
        W_ = N.RESAMPLE_WINDOW
        refused += [(good(flags=W_, lo=lo, hi=hi), True, None, INVALID, "window") for lo, hi in ((0.5, 0.5), (0.6, 0.5), (float("nan"), 1.0), (0.0, float("inf")), (-float("inf"), 0.0))]
        refused.append((good(flags=W_, lo=0.0, hi=1e-45, format=N.FMT_R16_UNORM), True, None, INVALID, "not finite in f32"))
        refused.append((good(), False, None, INVALID, "neither dense_out nor VK_RESAMPLE_INSTALL"))
        refused.append((good(flags=N.RESAMPLE_INSTALL, layout=7), True, None, INVALID, "unknown layout"))
        refused.append((good(), True, N.VkVoxelBox(5, 0, 0, 4, 20, 7), INVALID, "inverted or leaves the volume"))
        refused.append((good(), True, N.VkVoxelBox(0, 0, 0, 41, 20, 7), INVALID, "inverted or leaves the volume"))
        refused.append((good(), True, N.VkVoxelBox(3, 3, 3, 3, 9, 7), INVALID, "the box is empty"))
        refused.append((good(flags=N.RESAMPLE_CLIP_BOX), True, N.VkVoxelBox(0, 0, 0, 4, 4, 4), INVALID, "box must be NULL"))
        refused.append((good(mode=N.RESAMPLE_AREA, dims=(C.c_uint32 * 3)(2, 10, 7)), True, None, UNSUPPORTED, "VK_RESAMPLE_MAX_RATIO"))          # 40 -> 2
        refused.append((good(flags=N.RESAMPLE_INSTALL, format=N.FMT_R16_UNORM, layout=V.LAYOUT_PACKED_PAIRS), True, None, UNSUPPORTED, "PACKED_PAIRS"))
        refused.append((good(flags=N.RESAMPLE_INSTALL, format=N.FMT_R16_UNORM, layout=V.LAYOUT_BRICKED), True, None, UNSUPPORTED, "R16_UNORM"))
        refused.append((good(flags=N.RESAMPLE_INSTALL, dims=(C.c_uint32 * 3)(8193, 1, 1)), True, None, UNSUPPORTED, "8192"))
        for req, dense, box, status, word in refused:
            rc, msg = raw(ctx, req, dense, box)
            assert rc == status and word in msg and msg.startswith("resample: ") and untouched(), (word, rc, msg)
            assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty
        # what is accepted: the bounds themselves, junk in lo / hi without the flag and in layout without an install
        assert raw(ctx, good(mode=N.RESAMPLE_AREA, dims=(C.c_uint32 * 3)(3, 2, 1)))[0] == 0 and not untouched()   # 40 -> 3, 20 -> 2, 7 -> 1
        assert tuple(res.dims) == (3, 2, 1) and res.format == 0 and res.layout == 0
        assert raw(ctx, good(lo=float("nan"), hi=float("nan"), layout=99))[0] == 0 and not untouched()
        assert raw(ctx, good(flags=N.RESAMPLE_CLIP_BOX))[0] == 0 and tuple(res.dims) == (20, 10, 7) and res.box.x1 == 40   # no clip box set: the whole volume
        assert _info(V, ctx) == info and _empty_fraction(V, ctx) == empty and _same_frame(_frame(V, ctx), frame)
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            for r in (good(), good(mode=N.RESAMPLE_NEAREST, flags=N.RESAMPLE_INSTALL)):
                rc, msg = raw(ctx, r)
                assert rc == UNSUPPORTED and msg.startswith("resample: ") and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, good())
        assert rc == UNSUPPORTED and msg.startswith("resample: ") and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and msg.startswith("resample: ") and "no volume" in msg and untouched()
    finally:
        ctx.close()


# ---- 6. the Python wrappers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_python_wrappers_against_both_references(V, lib, kind, layout):  # noqa: F811
    d = (37, 10, 9)
    vol = RC.noise(d, kind, 12)
    whole = (0, 0, 0) + d

    def both(box, mode, dims, out, window):
        a = RH.restate(lib, vol, kind, box, mode, dims, out, window)
        assert RH.differences(a, NR.resample(vol, kind, box, mode, dims, out, window)) == ""
        return a

    ctx = _ctx(V, vol, kind, layout)
    try:
        info = _info(V, ctx)
        # resample_volume: dims, out without install
        got, res = ctx.resample_volume((64, 7, 3), install=False, out=True)
        assert RH.differences(got, both(whole, "linear", (64, 7, 3), kind, None)) == "" and tuple(res.dims) == (64, 7, 3) and res.layout == 0
        # scale, a box, another format under a window
        got, res = ctx.resample_volume(scale=(0.5, 2.0, 1.0), box=((4, 1, 2), (34, 9, 8)), mode="area", fmt="u8", window=(0.2, 0.7), install=False, out=True)
        assert tuple(res.dims) == (15, 16, 6) and got.dtype == np.uint8
        assert RH.differences(got, both((4, 1, 2, 34, 9, 8), "area", (15, 16, 6), "u8", (0.2, 0.7))) == ""
        # downsample_volume and isotropic_volume
        got, res = ctx.downsample_volume(2, install=False, out=True)
        assert tuple(res.dims) == (19, 5, 5) and RH.differences(got, both(whole, "area", (19, 5, 5), kind, None)) == ""
        got, res = ctx.isotropic_volume((1.0, 1.0, 2.5), install=False, out=True)
        assert tuple(res.dims) == (37, 10, 22) and RH.differences(got, both(whole, "linear", (37, 10, 22), kind, None)) == ""
        with pytest.raises(V.VokselisError) as e:
            ctx.resample_volume((2, 10, 9), mode="area")  # 37 -> 2
        assert e.value.code == UNSUPPORTED
        assert _info(V, ctx) == info
        # crop_volume("clip"): installs the clip box's voxels and turns the box off
        lo3, hi3 = (0.13, 0.0, 0.21), (0.81, 0.77, 1.0)
        ctx.set_clip_box(lo3, hi3)
        cb = RC.clip_voxel_box(lo3, hi3, d)
        nb = (cb[3] - cb[0], cb[4] - cb[1], cb[5] - cb[2])
        got, res = ctx.crop_volume("clip", out=True)
        assert RH.differences(got, NR.crop(vol, cb)) == "" and RH.differences(got, both(cb, "nearest", nb, kind, None)) == ""
        assert (res.box.x0, res.box.y0, res.box.z0, res.box.x1, res.box.y1, res.box.z1) == cb
        assert _info(V, ctx) == (nb, info[1], info[2]) and ctx.clip_box is None
        # an explicit crop of the crop; nothing requested is refused before the library sees it
        res = ctx.crop_volume(((1, 1, 1), (9, 7, 5)))
        assert tuple(res.dims) == (8, 6, 4) and _info(V, ctx)[0] == (8, 6, 4)
        got, _ = ctx.resample_volume(mode="nearest", install=False, out=True)
        assert RH.differences(got, NR.crop(NR.crop(vol, cb), (1, 1, 1, 9, 7, 5))) == ""
        with pytest.raises(ValueError):
            ctx.resample_volume((4, 4, 4), install=False, out=False)
    finally:
        ctx.close()


# ---- 7. the C++ host ------------------------------------------------------------------------------------------------------------------
def test_bonsai_crops_downsamples_converts_and_saves_the_new_volume(V, lib, tmp_path):  # noqa: F811
    """bonsai --raw-u16 --crop --downsample 2 --to-u8 0.1 0.6 --save-raw --histogram: the file is the restatement's chain -- the crop
    (NEAREST), the mean of 2^3 voxels (AREA), the window into u8 (NEAREST with the map) -- and --histogram counts that volume."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(RH.ROOT, "vokselis_amd", "_lib", "bonsai")
    d = (37, 10, 9)
    vol = RC.noise(d, "u16", 31)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    args = [exe, "--raw-u16", str(src), "--dims"] + [str(v) for v in d] + ["--crop", "3", "1", "0", "36", "9", "9", "--downsample", "2", "--to-u8", "0.1", "0.6", "--save-raw", str(dst),
                                                                         "--histogram", "256"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    box = (3, 1, 0, 36, 9, 9)
    crop = RH.restate(lib, vol, "u16", box, "nearest", (33, 8, 9), "u16", None)
    assert RH.differences(crop, NR.crop(vol, box)) == ""
    half = RH.restate(lib, crop, "u16", (0, 0, 0, 33, 8, 9), "area", (17, 4, 5), "u16", None)
    want = RH.restate(lib, half, "u16", (0, 0, 0, 17, 4, 5), "nearest", (17, 4, 5), "u8", (0.1, 0.6))
    got = np.fromfile(dst, np.uint8).reshape(want.shape)
    assert RH.differences(got, want) == ""
    lines = r.stdout.splitlines()
    assert "crop: volume 33 x 8 x 9 R16_UNORM" in lines and "downsample: volume 17 x 4 x 5 R16_UNORM" in lines and "to-u8: volume 17 x 4 x 5 R8_UNORM" in lines
    assert any(line.startswith("resampled volume: %d bytes" % want.nbytes) for line in lines)
    counts = {int(a): int(b) for a, b in (line.split() for line in lines if len(line.split()) == 2 and line.split()[0].isdigit())}
    ref = np.bincount(want.ravel().astype(np.int64), minlength=256)
    assert counts == {i: int(n) for i, n in enumerate(ref) if n}


def test_bonsai_crop_clip_consumes_the_clip_box(V, tmp_path):  # noqa: F811
    """bonsai --clip ... --crop clip --save-raw with nothing that marches under a clip box: the crop takes the box and turns it off, so
    the plain render that follows needs no --tf / --mip / --iso."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(RH.ROOT, "vokselis_amd", "_lib", "bonsai")
    d = (37, 10, 9)
    vol = RC.noise(d, "u8", 33)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    lo3, hi3 = (0.13, 0.0, 0.21), (0.81, 0.77, 1.0)
    args = [exe, "--frames", "1", "--size", "64x64", "--raw", str(src), "--dims"] + [str(v) for v in d] + ["--clip"] + [str(v) for v in lo3 + hi3] + ["--crop", "clip", "--save-raw", str(dst)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = NR.crop(vol, RC.clip_voxel_box(lo3, hi3, d))
    assert RH.differences(np.fromfile(dst, np.uint8).reshape(want.shape), want) == ""
