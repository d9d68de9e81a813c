"""vk_split_components on the MI355X.  Every shared case (tests/split_cases.py) on every layout its format supports:
labels, region table, every field of the result and dense_out bitwise equal to the C restatement, with the grids capped so that the
grid-stride loops run; a truncated table is a prefix; radius 0 against vk_label_components on the device; VK_SPLIT_INSTALL read back,
refused inside an open frame, and followed by label_components / keep_components(seeds); the refusals with their status and text; two
runs with identical bytes; the Python wrapper.  There is no tolerance anywhere: every comparison is of integers or of stored bits."""
import ctypes as C
import math

import numpy as np
import pytest

import label_cases as LC
import label_helpers as LH
import split_cases as SC
import split_helpers as SH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
W, H = 64, 64


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("split_fuzz_gpu"))


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
    return next(c for c in SC.cases() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))


def _held(V, ctx, vol, kind):  # noqa: F811
    """The volume the context holds now, as a dense array: KEEP_ALL over every value with nothing to fill."""
    c = LC.Case("", "", vol, kind, -math.inf, math.inf, 6, None, None, "all", 0, (), False, 0.0)
    rc, got = LH.run(V, ctx, c, labels=False)
    assert rc == 0
    return got[3]


@pytest.mark.parametrize("kind, layout", [(k, l) for k in ("u8", "u16", "f16") for l in LH.LAYOUTS[k]])
def test_every_case_is_bitwise_the_restatement(V, expected, kind, layout):  # noqa: F811
    cases = [c for c in SC.cases() if c.kind == kind]
    assert len(cases) >= 10
    ctx = _ctx(V)
    try:
        uploaded = None
        for i, c in enumerate(cases):
            if c.vol_id != uploaded:
                LH.upload(V, ctx, c.vol, kind, layout)
                uploaded = c.vol_id
            ctx.set_param("label_max_blocks", (0, 1, 3)[i % 3])  # the grid-stride loops over tiles and chunks on small volumes too
            ctx.set_param("dist_max_blocks", (0, 2, 1)[i % 3])
            if c.clip is not None:
                ctx.set_clip_box(*c.clip)
            rc, got = SH.run(V, ctx, c)
            if c.clip is not None:
                ctx.set_clip_box(None)
            assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
            assert LH.differences(got, expected[c.name][:4]) == "", (c.name, layout)
    finally:
        ctx.close()


def test_a_truncated_table_is_a_prefix_and_absent_outputs_change_nothing(V, expected):  # noqa: F811
    c = _case("percolation at density 0.62", "u8")
    want = expected[c.name]
    n = int(want[2][0])
    assert n > 100
    ctx = _ctx(V, c.vol, "u8", "PACKED")
    try:
        for cap in (1, 7, n - 1, n, n + 5):
            rc, got = SH.run(V, ctx, c, cap=cap, dense=False, labels=(cap == 7))
            assert rc == 0 and len(got[1]) == min(cap, n) and (got[1] == want[1][:cap]).all() and (got[2] == want[2]).all(), cap
        N = V.native
        req, _ = SH.request(c)
        res = N.VkSplitResult()
        assert N.lib().vk_split_components(ctx.handle, C.byref(req), None, None, None, 0, None, C.byref(res)) == 0  # the totals alone
        assert (SH.result_array(res) == want[2]).all()
        lab = np.zeros(c.vol.shape, np.uint32)
        assert N.lib().vk_split_components(ctx.handle, C.byref(req), None, lab.ctypes.data, None, 0, None, None) == 0  # the labels alone
        assert (lab == want[0]).all()
    finally:
        ctx.close()


def test_radius_zero_and_an_empty_marker_set_are_label_components_on_the_device(V):  # noqa: F811
    for c in (_case("fixed", "u8", radius=0.0), _case("K empty", "f16"), _case("specials", "f16", radius=0.0, conn=6)):
        ctx = _ctx(V, c.vol, c.kind, "LINEAR")
        try:
            rc, got = SH.run(V, ctx, c, dense=False)
            lc = LC.Case("", "", c.vol, c.kind, c.lo, c.hi, c.conn, c.box, None, "all", 0, (), False, 0.0)
            rc2, ref = LH.run(V, ctx, lc, dense=False)
            assert rc == 0 and rc2 == 0
            assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and got[2][0] == ref[2][0] and got[2][1] == ref[2][1], c.name
            assert int(got[2][6]) == 0  # nothing is cut
        finally:
            ctx.close()


def test_two_runs_give_identical_bytes(V):  # noqa: F811
    c = _case("grains", "u16", conn=26)
    ctx = _ctx(V, c.vol, "u16", "LINEAR")
    try:
        runs = [SH.run(V, ctx, c) for _ in range(2)]
        assert runs[0][0] == 0 and runs[1][0] == 0
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][1], runs[1][1]))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_install_then_label_and_keep_seeds(V, expected, kind, layout):  # noqa: F811
    """The installed volume read back is dense_out; the dimensions, format and layout stay; an install inside an open frame is refused and
    the old volume kept; label_components of the cut volume never joins two regions; keep_components(seeds) with a region's anchor
    returns a subset of that region."""
    c = _case("grains", kind, conn=6)
    labels, table, result, dense, _ = expected[c.name]
    assert int(result[0]) >= 2 and int(result[6]) > 0
    ctx = _ctx(V, c.vol, kind, layout)
    try:
        info = ctx._volume_dtype()
        fid = ctx.frame_begin()
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
        rc, _ = SH.run(V, ctx, c, install=True)
        msg = V.native.lib().vk_last_error(ctx.handle).decode()
        ctx.frame_end()
        ctx.read_frame(fid)
        assert rc == INVALID and "a frame is being recorded" in msg
        assert LH.differences((None, None, None, _held(V, ctx, c.vol, kind)), (None, None, None, np.ascontiguousarray(c.vol))) == ""
        rc, got = SH.run(V, ctx, c, install=True)
        assert rc == 0 and LH.differences(got, expected[c.name][:4]) == ""
        assert ctx._volume_dtype() == info
        assert LH.differences((None, None, None, _held(V, ctx, c.vol, kind)), (None, None, None, dense)) == ""
        comps = ctx.label_components(c.lo, c.hi, connectivity=c.conn, labels=True)
        cut = (labels != 0) & (comps.labels == 0)
        assert int(cut.sum()) == int(result[6])
        for k in range(1, comps.n + 1):
            assert len(np.unique(labels[comps.labels == k])) == 1, k     # a component of the cut volume lies inside one region
        region = int(np.argmax(table[:, 0])) + 1
        a = int(table[region - 1, 1])
        seed = (a % c.vol.shape[2], a // c.vol.shape[2] % c.vol.shape[1], a // (c.vol.shape[2] * c.vol.shape[1]))
        kept, res = ctx.keep_components(c.lo, c.hi, keep="seeds", seeds=[seed], install=False, out=True)
        inside = LH.raw(kept) != LH.raw(np.zeros(1, kept.dtype))[0]
        assert res.n_kept_components == 1 and inside.any() and (labels[inside] == region).all()
    finally:
        ctx.close()


def test_every_refusal_returns_its_status_and_text_and_leaves_everything_alone(V):  # noqa: F811
    N = V.native
    vol = np.random.default_rng(5).integers(0, 256, (7, 20, 33)).astype(np.uint8)
    out = np.full(vol.shape, 0xAB, np.uint8)
    lab = np.full(vol.shape, 0xABABABAB, np.uint32)
    comps = (N.VkComponent * 4)()
    res = N.VkSplitResult()
    res.n_regions = res.n_cut = 9

    def raw(ctx, req, box=None, labels=True, components=False, cap=4, dense=True, result=True):
        out[...] = 0xAB
        lab[...] = 0xABABABAB
        rc = N.lib().vk_split_components(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, lab.ctypes.data if labels else None,
                                         comps if components else None, cap, out.ctypes.data if dense else None, C.byref(res) if result else None)
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((out == 0xAB).all() and (lab == 0xABABABAB).all() and res.n_regions == 9 and res.n_cut == 9)

    def good(**kw):
        r = N.VkSplitRequest()
        r.lo, r.hi, r.connectivity, r.radius = 0.5, math.inf, 6, 1.0
        r.spacing[0] = r.spacing[1] = r.spacing[2] = 1
        for k, v in kw.items():
            if k == "spacing":
                r.spacing[0], r.spacing[1], r.spacing[2] = v
            else:
                setattr(r, k, v)
        return r

    ctx = _ctx(V, vol, "u8", "PACKED")
    try:
        before = _held(V, ctx, vol, "u8")
        refused = [(None, {}, "the request is NULL"), (good(lo=math.nan), {}, "NaN"), (good(hi=math.nan), {}, "NaN"), (good(lo=0.6, hi=0.5), {}, "lo > hi")]
        refused += [(good(fill_out=f), {}, "fill_out is not finite") for f in (math.nan, math.inf, -math.inf)]
        refused += [(good(connectivity=k), {}, "connectivity must be 6, 18 or 26") for k in (0, 4, 8, 27, 0xffffffff)]
        refused += [(good(flags=f), {}, "unknown flag") for f in (4, 8, 1 << 31, 7)]
        refused += [(good(pad=1), {}, "pad must be 0")]
        refused += [(good(spacing=s), {}, "a spacing outside 1 .. VK_DIST_MAX_SPACING") for s in ((0, 1, 1), (1, 65, 1), (1, 1, 0xffffffff))]
        refused += [(good(radius=r), {}, "the radius is not finite, is negative") for r in (math.nan, math.inf, -1.0, 65536.0)]
        refused += [(good(), dict(components=True, cap=0), "cap_components == 0")]
        refused += [(good(), dict(labels=False, dense=False, result=False), "the result would go nowhere")]
        refused += [(good(fill_out=0.5), {}, "the cut would cut nothing"), (good(fill_out=7.0), {}, "the cut would cut nothing"), (good(lo=-math.inf, hi=0.6, fill_out=0.0), {}, "the cut would cut nothing"),
                    (good(fill_out=1.0, flags=N.SPLIT_INSTALL), dict(dense=False), "the cut would cut nothing")]
        refused += [(good(), dict(box=N.VkVoxelBox(5, 0, 0, 4, 20, 7)), "the box is inverted or leaves the volume"), (good(), dict(box=N.VkVoxelBox(0, 0, 0, 34, 20, 7)), "leaves the volume"),
                    (good(flags=N.SPLIT_CLIP_BOX), dict(box=N.VkVoxelBox(0, 0, 0, 1, 1, 1)), "VK_SPLIT_CLIP_BOX takes the box from the clip box: box must be NULL")]
        for req, kw, word in refused:
            rc, msg = raw(ctx, req, **kw)
            assert rc == INVALID and word in msg and msg.startswith("vk_split_components: ") and untouched(), (word, rc, msg)
        rc, msg = raw(ctx, good(spacing=(64, 64, 64), radius=0.0), dense=False)   # (64 * 32)^2 + ... fits; a larger pitch times the extent does not
        assert rc == 0
        res.n_regions = res.n_cut = 9
        # a fill inside the range is accepted where no volume is written
        assert raw(ctx, good(fill_out=0.9), dense=False)[0] == 0
        res.n_regions = res.n_cut = 9
        assert LH.differences((None, None, None, _held(V, ctx, vol, "u8")), (None, None, None, before)) == ""
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, "u8", layout)
        try:
            rc, msg = raw(ctx, good())
            assert rc == UNSUPPORTED and msg.startswith("split: ") and "needs a scalar LINEAR, PACKED or PACKED_PAIRS volume" in msg and untouched(), (layout, msg)
        finally:
            ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, good())
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()
    big = np.zeros((1, 1, 2000), np.uint8)  # (64 * 1999)^2 > 0xFFFFFFFE
    ctx = _ctx(V, big, "u8", "LINEAR")
    try:
        rc, msg = raw(ctx, good(spacing=(64, 1, 1)), labels=False, dense=False)
        assert rc == UNSUPPORTED and msg.startswith("split: ") and "would not fit in 32 bits" in msg and untouched()
    finally:
        ctx.close()


def test_python_wrapper_against_the_restatement(V, lib, expected):  # noqa: F811
    c = _case("fixed", "u8", radius=6.0)
    labels, table, result, dense, _ = expected[c.name]
    ctx = _ctx(V, c.vol, "u8", "PACKED")
    try:
        r = ctx.split_components(0.5, radius=6.0, labels=True, out=True)
        assert r.n == 3 and (r.labels == labels).all() and (r.sizes == table[:, 0]).all() and (r.first == table[:, 1]).all() and (r.boxes == table[:, 2:]).all()
        assert sorted(int(s) for s in r.sizes) == [7, 1979, 2063] and list(r.largest(1)) == [int(np.argmax(table[:, 0])) + 1]
        assert (r.n_foreground, r.n_markers, r.n_marker_voxels, r.n_residue_regions, r.n_residue_voxels, r.n_cut, r.rounds) == tuple(int(v) for v in result[1:])
        assert r.rounds == 11 and r.n_markers == 2 and (r.dense == dense).all()
        assert ctx.split_components(0.5, radius=6.0).labels is None and ctx.label_components(0.5).n == 2   # nothing was installed
        ctx.split_components(0.5, radius=6.0, install=True)
        assert ctx.label_components(0.5).n >= 3
        with pytest.raises(ValueError):
            ctx.split_components(0.5, radius=-1.0)
        with pytest.raises(V.VokselisError) as e:
            ctx.split_components(0.5, radius=1.0, connectivity=7)
        assert e.value.code == INVALID
    finally:
        ctx.close()
