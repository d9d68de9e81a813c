"""vk_measure_components on the MI355X.  Every shared case (tests/measure_cases.py) on every layout its format
supports, from both label sources: the records bitwise equal to the C restatement, with the grids capped so that the grid-stride loops
run; the same records with the grid capped to 1, 2 and 7 blocks; a timed call's outputs equal to the untimed call's; vk_label_components'
labels_out fed back in gives the records of the call that labels itself, and n_voxels / first / box are that call's table; a truncated
table is a prefix; an id above max_label is refused; the refusals with their status and text.  There is no tolerance anywhere: every
comparison is of integers."""
import ctypes as C
import math

import numpy as np
import pytest

import label_cases as LC
import label_helpers as LH
import measure_cases as MC
import measure_helpers as MH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("measure_fuzz_gpu")
    return MH.build_restatement(d), LH.build_restatement(d)


@pytest.fixture(scope="module")
def expected(libs):
    """Per case: (table, n_foreground) of the C restatement, computed once and left unchanged."""
    out = {}
    for c in MC.cases():
        table, fg = MH.restate_case(libs[0], libs[1], c)
        table.setflags(write=False)
        out[c.name] = (table, fg)
    return out


def _ctx(V, vol=None, kind=None, layout="PACKED"):  # noqa: F811
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        if vol is not None:
            LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
    except BaseException:
        ctx.close()
        raise
    return ctx


def _case(word, kind, **where):
    return next(c for c in MC.cases() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))


def _error(V, ctx):  # noqa: F811
    return V.native.lib().vk_last_error(ctx.handle).decode()


def _result(res):
    return (int(res.n_regions), int(res.n_foreground), int(res.records_written), int(res.scale))


SCALE = {"u8": 255, "u16": 65535, "f16": 1 << 24}


@pytest.mark.parametrize("kind, layout", [(k, l) for k in ("u8", "u16", "f16") for l in LH.LAYOUTS[k]])
def test_every_case_from_both_label_sources_is_bitwise_the_restatement(V, libs, expected, kind, layout):  # noqa: F811
    cases = [c for c in MC.cases() if c.kind == kind]
    assert len(cases) >= 10
    ctx = _ctx(V)
    try:
        uploaded = None
        for i, c in enumerate(cases):
            if c.vol_id != uploaded:
                LH.upload(V, ctx, c.vol, kind, layout)
                uploaded = c.vol_id
            ctx.set_param("label_max_blocks", (0, 1, 3)[i % 3])  # the grid-stride loops over tiles and chunks on small volumes too
            table, fg = expected[c.name]
            if c.clip is not None:
                ctx.set_clip_box(*c.clip)
            rc, got, res = MH.run(V, ctx, c)
            if c.clip is not None:
                ctx.set_clip_box(None)
            assert rc == 0, (c.name, _error(V, ctx))
            assert MH.differences(got, table) == "", (c.name, layout)
            assert _result(res) == (len(table), fg, len(table), SCALE[kind]), (c.name, layout)
            if c.labels is None:
                # the other source: the label restatement's array as labels_in.  No region at all: max_label 1 and one empty record
                labels, n, _ = MH.case_labels(libs[1], c)
                want = table if n else MH.restate(libs[0], c.vol, kind, labels, 1)[0]
                rc, got, res = MH.run(V, ctx, c, labels=labels, max_label=max(n, 1))
                assert rc == 0, (c.name, _error(V, ctx))
                assert MH.differences(got, want) == "", (c.name, layout, "labels_in")
                assert _result(res) == (max(n, 1), fg, max(n, 1), SCALE[kind]), (c.name, layout)
    finally:
        ctx.close()


@pytest.mark.parametrize("word, kind, layout", [("one region fills the volume", "u8", "PACKED_PAIRS"), ("one region fills the volume", "f16", "LINEAR"),
                                               ("isolated voxels", "u16", "PACKED"), ("regions that share faces", "f16", "PACKED"),
                                               ("a caller's scattered segmentation", "u8", "LINEAR")])
def test_the_records_do_not_depend_on_the_launch_shape(V, expected, word, kind, layout):  # noqa: F811
    c = _case(word, kind)
    ctx = _ctx(V, c.vol, kind, layout)
    try:
        for blocks in (1, 2, 7, 0):
            ctx.set_param("label_max_blocks", blocks)
            rc, got, _ = MH.run(V, ctx, c)
            assert rc == 0 and MH.differences(got, expected[c.name][0]) == "", (c.name, blocks)
    finally:
        ctx.close()


def test_a_timed_call_gives_the_untimed_calls_outputs(V, expected):  # noqa: F811
    N = V.native
    for c, phases in ((_case("odd dimensions", "f16", conn=6), (1, 2, 3, 4, 5)), (_case("unused ids", "u8"), (1, 4, 5))):
        ctx = _ctx(V, c.vol, c.kind, "PACKED")
        try:
            for k in phases:
                ctx.set_param("measure_timing", k)
                rc, got, res = MH.run(V, ctx, c)
                ms = C.c_float(-1.0)
                assert rc == 0 and MH.differences(got, expected[c.name][0]) == "" and _result(res)[1] == expected[c.name][1], (c.name, k)
                assert N.lib().vk_timer_elapsed_ms(ctx.handle, C.byref(ms)) == 0 and math.isfinite(ms.value) and ms.value >= 0.0, (c.name, k)
            ctx.set_param("measure_timing", 0)
        finally:
            ctx.close()


@pytest.mark.parametrize("kind", ["u8", "u16", "f16"])
def test_label_components_labels_fed_back_give_the_same_records_and_its_table(V, kind):  # noqa: F811
    c = _case("regions of every size", kind)
    ctx = _ctx(V, c.vol, kind, "PACKED")
    try:
        lc = LC.Case("", "", c.vol, kind, c.lo, c.hi, c.conn, None, None, "all", 0, (), False, 0.0)
        rc, (labels, table, result, _) = LH.run(V, ctx, lc, dense=False)
        assert rc == 0 and int(result[0]) > 3
        rc, own, res = MH.run(V, ctx, c)
        rc2, fed, res2 = MH.run(V, ctx, c, labels=labels, max_label=int(result[0]))
        assert rc == 0 and rc2 == 0 and MH.differences(fed, own) == "" and _result(res) == _result(res2)
        assert (own[:, :8] == table).all() and int(res.n_foreground) == int(result[1])
    finally:
        ctx.close()


def test_a_truncated_table_is_a_prefix_and_the_totals_alone(V, expected):  # noqa: F811
    c = _case("odd dimensions", "u8", conn=6)
    want, fg = expected[c.name]
    n = len(want)
    assert n > 100
    ctx = _ctx(V, c.vol, "u8", "PACKED")
    try:
        for cap in (1, 7, n - 1, n, n + 5):
            rc, got, res = MH.run(V, ctx, c, cap=cap)
            assert rc == 0 and (got == want[:cap]).all() and _result(res) == (n, fg, min(cap, n), 255), cap
        N = V.native
        req, _ = MH.request(c)
        res = N.VkMeasureResult()
        assert N.lib().vk_measure_components(ctx.handle, C.byref(req), None, None, None, 0, C.byref(res)) == 0  # the totals alone
        assert _result(res) == (n, fg, 0, 255)
        regions = (N.VkRegion * n)()
        assert N.lib().vk_measure_components(ctx.handle, C.byref(req), None, None, regions, n, None) == 0      # the records alone
        assert (MH.table_array(regions, n) == want).all()
    finally:
        ctx.close()


def test_an_id_above_max_label_is_refused_after_the_upload(V, expected):  # noqa: F811
    c = _case("unused ids", "u16")
    ctx = _ctx(V, c.vol, "u16", "LINEAR")
    try:
        top = int(c.labels.max())
        N = V.native
        regions = (N.VkRegion * 16)()
        C.memset(regions, 0xAB, C.sizeof(regions))
        res = N.VkMeasureResult()
        res.n_regions = 9
        req, _ = MH.request(c)
        req.max_label = top - 1
        rc = N.lib().vk_measure_components(ctx.handle, C.byref(req), None, c.labels.ctypes.data, regions, 16, C.byref(res))
        assert rc == INVALID and _error(V, ctx) == "vk_measure_components: labels_in holds an id above max_label"
        assert bytes(regions) == b"\xab" * C.sizeof(regions) and res.n_regions == 9
        rc, got, _ = MH.run(V, ctx, c, max_label=top)  # the largest id itself is fine; ids above it then do not exist
        assert rc == 0 and (got == expected[c.name][0][:top]).all()
    finally:
        ctx.close()


def test_every_refusal_returns_its_status_and_text_and_leaves_everything_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 33)).astype(np.uint8)
    lab = np.ones(vol.shape, np.uint32)
    regions = (N.VkRegion * 4)()
    res = N.VkMeasureResult()

    def raw(ctx, req, box=None, labels=False, want_regions=True, cap=4, result=True):
        C.memset(regions, 0xAB, C.sizeof(regions))
        res.n_regions = res.records_written = 9
        rc = N.lib().vk_measure_components(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, lab.ctypes.data if labels else None,
                                           regions if want_regions else None, cap, C.byref(res) if result else None)
        return rc, _error(V, ctx)

    def untouched():
        return bytes(regions) == b"\xab" * C.sizeof(regions) and res.n_regions == 9 and res.records_written == 9

    def good(**kw):
        r = N.VkMeasureRequest()
        r.lo, r.hi, r.connectivity = 0.5, math.inf, 6
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def with_labels(**kw):
        r = N.VkMeasureRequest()
        r.max_label = 1
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        refused = [(None, {}, "the request is NULL"), (good(lo=math.nan), {}, "NaN"), (good(hi=math.nan), {}, "NaN"), (good(lo=0.6, hi=0.5), {}, "lo > hi")]
        refused += [(good(connectivity=k), {}, "connectivity must be 6, 18 or 26") for k in (0, 4, 8, 27, 0xffffffff)]
        refused += [(good(flags=f), {}, "unknown flag") for f in (2, 4, 1 << 31, 3)]
        refused += [(good(pad=1), {}, "pad must be 0")]
        refused += [(good(), dict(cap=0), "cap_regions == 0")]
        refused += [(good(), dict(want_regions=False, result=False), "the result would go nowhere")]
        refused += [(good(max_label=3), {}, "max_label != 0 without labels_in")]
        refused += [(with_labels(lo=0.5, hi=0.5), dict(labels=True), "must be 0 with labels_in"), (with_labels(hi=1.0), dict(labels=True), "must be 0 with labels_in"),
                    (with_labels(connectivity=6), dict(labels=True), "must be 0 with labels_in"),
                    (with_labels(flags=N.MEASURE_CLIP_BOX), dict(labels=True), "a box or VK_MEASURE_CLIP_BOX with labels_in"),
                    (with_labels(), dict(labels=True, box=N.VkVoxelBox(0, 0, 0, 1, 1, 1)), "a box or VK_MEASURE_CLIP_BOX with labels_in"),
                    (with_labels(max_label=0), dict(labels=True), "max_label == 0 with labels_in"),
                    (with_labels(max_label=vol.size + 1), dict(labels=True), "max_label exceeds the voxel count")]
        refused += [(good(), dict(box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the box is inverted or leaves the volume"), (good(), dict(box=N.VkVoxelBox(0, 0, 0, 34, 20, 7)), "leaves the volume"),
                    (good(flags=N.MEASURE_CLIP_BOX), dict(box=N.VkVoxelBox(0, 0, 0, 1, 1, 1)), "VK_MEASURE_CLIP_BOX takes the box from the clip box: box must be NULL")]
        for req, kw, word in refused:
            rc, msg = raw(ctx, req, **kw)
            assert rc == INVALID and word in msg and msg.startswith("vk_measure_components: ") and untouched(), (word, rc, msg)
        assert raw(ctx, with_labels(max_label=vol.size), labels=True, want_regions=False)[0] == 0  # the voxel count itself is allowed
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            rc, msg = raw(ctx, good())
            assert rc == UNSUPPORTED and msg.startswith("measure: ") and "needs a scalar LINEAR, PACKED or PACKED_PAIRS volume" in msg and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()
