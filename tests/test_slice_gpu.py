"""The slice pass on the MI355X through its entry points (vk_render_slice, vk_slice_values_info, vk_readback_slice_values,
vk_frame_slice_values, vk_slice_probe): the exact anchor against raw voxels on all seven layouts, tiles against the
frame, probes against the full-frame pass, the state the pass must ignore, the clip box, frame slots, resizes, device memory over
reshapes, and every refusal with its status.  The frames themselves are held to the restatement in tests/test_slice_fuzz_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import slice_helpers as SH
import test_slice_fuzz_cpu as AN  # the exact anchor's volumes, views and expectations
from gpu_helpers import V  # noqa: F401
from shadow_cases import two_balls

pytestmark = pytest.mark.gpu

W, H = 40, 24
INVALID, UNSUPPORTED = -1, -5
PLANE = np.array([[0.07, 0.93, 0.31], [0.024, -0.003, 0.007], [0.002, -0.041, 0.011], [0.004, 0.002, 0.03]], np.float32)  # oblique: its corners leave the cube
BOX = ((0.2, 0.1, 0.0), (0.8, 0.9, 0.7))
SEVEN = (("u8", "LINEAR"), ("u8", "PACKED"), ("u8", "PACKED_PAIRS"), ("f16", "LINEAR"), ("f16", "PACKED"), ("u16", "LINEAR"), ("u16", "PACKED"))


@pytest.fixture(scope="module")
def vol():
    v = two_balls((28, 22, 25))
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("slice_gpu"), O)


def _ctx(V, vol, layout="PACKED", size=(W, H), out_format=None):
    ctx = V.Context(size[0], size[1], backbuffer=size, out_format=V.OUT_RGBA32F if out_format is None else out_format)
    try:
        if vol is not None:
            kw = dict(fmt=V.FMT_R16_UNORM) if vol.dtype == np.uint16 else {}
            V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout), **kw)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _slice(V, samples=1, reduce="max", plane=PLANE):
    return V.Slice.raw(plane[0], plane[1], plane[2], plane[3], samples, reduce)


def _frame(ctx, s, tile=None):
    ctx.render_slice(s, tile, values=True)
    return ctx.read_backbuffer().copy(), ctx.read_slice_values()


def _code(V, fn):
    with pytest.raises(V.VokselisError) as e:
        fn()
    return e.value.code, str(e.value)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kind, layout", SEVEN)
def test_exact_anchor_against_raw_voxels(V, kind, layout):  # noqa: F811
    """Power-of-two dims and the orthogonal views at the volume's own size: every position is a texel centre exactly, so x is the raw voxel
    as a float at every pixel, and a MEAN over an odd number of planes is f32(sum) * rn.  No restatement involved."""
    data = AN.anchor_volumes()[kind]
    checked = 0
    for name, build, (w, h), plane_of, _, n_axis in AN.anchor_views(V):
        ctx = _ctx(V, data, layout, (w, h))
        try:
            for k in range(n_axis):
                ctx.render_slice(build(AN.ANCHOR_DIMS, k, w, h), values=True)
                val = ctx.read_slice_values()
                assert (val[..., 1] == 1.0).all(), (name, k)
                assert (_bits(val[..., 0]) == _bits(plane_of(data, k).astype(np.float32))).all(), (name, k)
                checked += 1
            for samples in (3, 5):
                k = n_axis // 2
                ctx.render_slice(build(AN.ANCHOR_DIMS, k, w, h, samples=samples, reduce="mean"), values=True)
                val = ctx.read_slice_values()
                assert (_bits(val[..., 0]) == _bits(AN.anchor_expected_mean(data, plane_of, k, samples, n_axis))).all(), (name, samples)
                checked += 1
        finally:
            ctx.close()
    assert checked == 4 + 8 + 16 + 6


def test_four_tiles_are_the_one_tile_frame(V, vol):  # noqa: F811
    for samples, reduce in ((1, "max"), (8, "mean")):
        s = _slice(V, samples, reduce)
        ctx = _ctx(V, vol)
        try:
            img, val = _frame(ctx, s)
            assert 100 < (val[..., 1] != 0).sum() < val[..., 1].size - 50  # part of the frame lies in the cube, part does not
        finally:
            ctx.close()
        ctx = _ctx(V, vol)
        try:
            for tile in ((0, 0, 13, 9), (13, 0, W - 13, 9), (-5, 9, 18, H), (13, 9, W, H - 9)):  # odd edges, one tile from off screen, two past the far edges
                ctx.render_slice(s, tile, values=True)
            assert (_bits(ctx.read_backbuffer()) == _bits(img)).all() and (_bits(ctx.read_slice_values()) == _bits(val)).all(), (samples, reduce)
        finally:
            ctx.close()


def test_probe_is_the_full_frame_record_and_the_restatements_position(V, lib, vol):  # noqa: F811
    s = _slice(V, 3, "min")
    _, ref_val, ref_pos, fl = SH.restate(lib, vol, W, H, PLANE, samples=3, reduce="min")
    # a plane on the face z = 1 for the face and corner pixels: P = (px / 32, py / 16, 1)
    face_plane = np.array([[0.0, 0.0, 1.0], [1 / 32, 0.0, 0.0], [0.0, 1 / 16, 0.0], [0.0, 0.0, 0.0]], np.float32)
    fs = _slice(V, plane=face_plane)
    _, fref_val, fref_pos, ffl = SH.restate(lib, vol, W, H, face_plane)
    ctx = _ctx(V, vol)
    try:
        _, val = _frame(ctx, s)
        ins = (fl & SH.INSIDE) != 0
        ys, xs = np.nonzero(ins)
        oy, ox = np.nonzero(~ins)
        pixels = [(int(xs[len(xs) // 2]), int(ys[len(ys) // 2])), (int(xs[0]), int(ys[0])), (int(ox[0]), int(oy[0])), (int(ox[-1]), int(oy[-1])), (0, 0), (W - 1, H - 1)]
        for x, y in pixels:
            p = ctx.slice_probe(s, x, y)
            assert bool(p.inside) == bool(ins[y, x]), (x, y)
            assert (_bits(np.array(p.pos[:], np.float32)) == _bits(ref_pos[y, x])).all(), (x, y)
            assert (_bits(np.float32(p.value)) == _bits(val[y, x, 0])).all() and SH.same_bits(np.float32(p.value), ref_val[y, x, 0]).all(), (x, y)
        # the probes wrote their own pixels' records again and nothing else
        assert (_bits(ctx.read_slice_values()) == _bits(val)).all()
        _, fval = _frame(ctx, fs)
        for x, y in ((0, 0), (32, 16), (32, 0), (0, 16), (7, 5), (33, 3), (5, 17)):  # the cube's corners on that face, a face pixel, two just outside
            p = ctx.slice_probe(fs, x, y)
            assert bool(p.inside) == bool((ffl[y, x] & SH.INSIDE) != 0) == (x <= 32 and y <= 16), (x, y)
            assert tuple(p.pos[:]) == (x / 32, y / 16, 1.0) and (_bits(np.array(p.pos[:], np.float32)) == _bits(fref_pos[y, x])).all()
            assert (_bits(np.float32(p.value)) == _bits(fval[y, x, 0])).all() and (_bits(np.float32(p.value)) == _bits(fref_val[y, x, 0])).all(), (x, y)
        assert _code(V, lambda: ctx.slice_probe(s, W, 0))[0] == INVALID and _code(V, lambda: ctx.slice_probe(s, 0, H))[0] == INVALID
        info = ctx.slice_values_info()
        assert (info["width"], info["height"]) == (W, H) and info["device_ptr"]
    finally:
        ctx.close()


def test_the_colour_frame_without_values_is_the_frame_with_them_and_allocates_no_surface(V, vol):  # noqa: F811
    for fmt in (V.OUT_RGBA32F, V.OUT_RGBA16F):
        ctx = _ctx(V, vol, out_format=fmt)
        try:
            for s in (_slice(V), _slice(V, 8, "max")):
                ctx.render_slice(s)
                plain = ctx.read_backbuffer().copy()
                code, msg = _code(V, ctx.read_slice_values)
                assert code == INVALID and "VK_SLICE_VALUES" in msg and _code(V, ctx.slice_values_info)[0] == INVALID
                assert (plain[..., :3] != 0).any()
            ctx.render_slice(s, values=True)
            assert (ctx.read_backbuffer().view(np.uint16) == plain.view(np.uint16)).all()
            assert (ctx.read_slice_values()[..., 1] != 0).any()
        finally:
            ctx.close()


def test_lighting_isosurface_shadows_projection_and_camera_are_without_influence(V, O, vol):  # noqa: F811
    s = _slice(V, 3, "mean")
    table = np.linspace(0.0, 1.0, 16 * 4, dtype=np.float32).reshape(16, 4)
    ctx = _ctx(V, vol)
    try:
        ctx.set_transfer_function(table, (0.1, 0.9))
        base = _frame(ctx, s)
        ctx.set_lighting(direction=(1.0, 0.3, 0.2), ambient=0.2, diffuse=0.8, specular=0.5, shininess=16.0)
        lit = _frame(ctx, s)
        ctx.set_isosurface(0.5, (0.1, 0.9, 0.4), 4)
        ctx.set_shadows(0.7, 2.0)
        iso = _frame(ctx, s)
        ctx.set_projection(V.PROJ_MAX)
        ctx.set_camera_blob(O.camera_blob(2.0, -0.4, 2.2, (0.4, 0.5, 0.6), W / H))
        rest = _frame(ctx, s)
        for other in (lit, iso, rest):
            assert (_bits(other[0]) == _bits(base[0])).all() and (_bits(other[1]) == _bits(base[1])).all()
        ctx.set_transfer_function(None)  # ... and the table is not: the grey ramp gives another frame from the same values
        grey = _frame(ctx, s)
        assert (_bits(grey[1]) == _bits(base[1])).all() and not (_bits(grey[0]) == _bits(base[0])).all()
    finally:
        ctx.close()


def test_clip_box_follows_the_restatement(V, lib, vol):  # noqa: F811
    s = _slice(V, 2, "max")
    want_free = SH.restate(lib, vol, W, H, PLANE, samples=2)
    want_cut = SH.restate(lib, vol, W, H, PLANE, samples=2, box=BOX)
    ctx = _ctx(V, vol)
    try:
        free = _frame(ctx, s)
        ctx.set_clip_box(*BOX)
        cut = _frame(ctx, s)
        ctx.set_clip_box(None)
        again = _frame(ctx, s)
    finally:
        ctx.close()
    assert (_bits(free[1]) == _bits(want_free[1])).all() and (_bits(cut[1]) == _bits(want_cut[1])).all() and (_bits(again[1]) == _bits(free[1])).all()
    assert (_bits(again[0]) == _bits(free[0])).all()
    n_free, n_cut = int((free[1][..., 1] != 0).sum()), int((cut[1][..., 1] != 0).sum())
    assert 0 < n_cut < n_free  # the box takes pixels away, and only takes away
    assert ((cut[1][..., 1] != 0) <= (free[1][..., 1] != 0)).all()
    gone = (free[1][..., 1] != 0) & (cut[1][..., 1] == 0)
    assert (cut[0][gone] == SH.CLEAR).all()


def test_a_pass_inside_a_frame_lands_in_that_frames_slot(V, vol):  # noqa: F811
    ctx = _ctx(V, vol)
    try:
        ctx.frames_in_flight(4)
        assert _code(V, ctx.read_slice_values)[0] == INVALID  # nothing has been rendered yet
        planes = [PLANE + np.array([[0.0, 0.0, 0.1 * k], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32) for k in range(4)]
        fids = []
        for k in range(4):
            fids.append(ctx.frame_begin())
            ctx.render_slice(_slice(V, plane=planes[k]), values=True)
            ctx.frame_end()
        got = [(ctx.read_frame(f).copy(), ctx.frame_slice_values(f)) for f in fids]
        ctx.frames_in_flight(1)
        for k in range(4):
            img, val = _frame(ctx, _slice(V, plane=planes[k]))
            assert (_bits(got[k][0]) == _bits(img)).all() and (_bits(got[k][1]) == _bits(val)).all(), k
        assert not (_bits(got[0][1]) == _bits(got[1][1])).all()
        # once a later frame has taken the slot, the frame's surface is gone
        ctx.frames_in_flight(4)
        ids = []
        for k in range(5):
            ids.append(ctx.frame_begin())
            ctx.render_slice(_slice(V), values=True)
            ctx.frame_end()
        code, msg = _code(V, lambda: ctx.frame_slice_values(ids[0]))
        assert code == INVALID and "later frame" in msg
        assert (ctx.frame_slice_values(ids[4])[..., 1] != 0).any()
        # a frame whose slot never saw a pass with values has no surface
        ctx.frames_in_flight(4)  # (a ring resize frees every slot's surface)
        f = ctx.frame_begin()
        ctx.render_slice(_slice(V))
        ctx.frame_end()
        code, msg = _code(V, lambda: ctx.frame_slice_values(f))
        assert code == INVALID and "no slice pass" in msg
    finally:
        ctx.close()


def test_a_resize_drops_the_surface_until_the_next_pass(V, vol):  # noqa: F811
    ctx = _ctx(V, vol)
    try:
        assert _code(V, ctx.read_slice_values)[0] == INVALID and _code(V, ctx.slice_values_info)[0] == INVALID
        ctx.render_slice(_slice(V), tile=(8, 8, 16, 8), values=True)
        first = ctx.read_slice_values()
        m = np.zeros((H, W), bool)
        m[8:16, 8:24] = True
        assert (_bits(first[~m]) == 0).all() and (first[m][:, 1] != 0).any()  # the allocation's fill: zero records everywhere the tile is not
        ctx.resize_backbuffer(W + 8, H - 8)
        assert _code(V, ctx.read_slice_values)[0] == INVALID and _code(V, ctx.slice_values_info)[0] == INVALID
        ctx.render_slice(_slice(V), values=True)
        val = ctx.read_slice_values()
        assert val.shape == (H - 8, W + 8, 2) and (val[..., 1] != 0).sum() > 100
        # a pitch larger than a row; a pitch smaller than one is refused
        rows = np.zeros((H - 8, (W + 8) * 2 + 6), np.float32)
        V.native.check(ctx.handle, V.native.lib().vk_readback_slice_values(ctx.handle, rows.ctypes.data, rows.strides[0]))
        assert (_bits(rows[:, :(W + 8) * 2].reshape(H - 8, W + 8, 2)) == _bits(val)).all() and (rows[:, (W + 8) * 2:] == 0).all()
        assert V.native.lib().vk_readback_slice_values(ctx.handle, rows.ctypes.data, (W + 8) * 8 - 4) == INVALID
    finally:
        ctx.close()


def test_every_refusal_returns_its_status_and_leaves_the_backbuffer_alone(V, vol):  # noqa: F811
    N = V.native
    ctx = _ctx(V, vol)
    try:
        ctx.render_slice(_slice(V))
        before = ctx.read_backbuffer().copy()

        def raw(s, flags=0):
            return N.lib().vk_render_slice(ctx.handle, C.byref(s) if s is not None else None, 0, 0, W, H, flags), N.lib().vk_last_error(ctx.handle).decode()

        def bent(**kw):
            s = _slice(V, 2, "max", plane=PLANE * np.float32(0.5))  # another frame: an accepted call would show in the backbuffer
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(s, k)[v[0]] = v[1]
                else:
                    setattr(s, k, v)
            return s

        refused = [(None, 0, "NULL")]
        for vec in ("origin", "du", "dv", "dn"):
            for bad in (float("nan"), float("inf"), -float("inf"), 1.0000001e6, -2e6):
                refused.append((bent(**{vec: (1, bad)}), 0, "not finite or beyond"))
        for n in (0, 257, 1 << 31):
            refused.append((bent(samples=n), 0, "samples"))
        for r in (-1, 3, 1 << 20):
            refused.append((bent(reduce=r), 0, "reduce"))
        for flags in (2, 4, 1 << 31, 3):
            refused.append((bent(), flags, "VK_SLICE_VALUES only"))
        for s, flags, word in refused:
            code, msg = raw(s, flags)
            assert code == INVALID and word in msg, (word, code, msg)
        assert (_bits(ctx.read_backbuffer()) == _bits(before)).all()
        assert _code(V, ctx.read_slice_values)[0] == INVALID  # ... and no refusal allocated the value surface
        # what is accepted: the bounds themselves, a garbage dn and reduce under samples == 1, an empty tile, a tile wholly off screen
        ok = _slice(V)
        ok.dn[0], ok.reduce = float("nan"), 77
        assert raw(ok)[0] == 0
        assert (_bits(ctx.read_backbuffer()) == _bits(before)).all()  # the same plane: the same frame
        edge = bent(origin=(0, 1e6), du=(2, -1e6))
        assert raw(edge)[0] == 0
        ctx.render_slice(_slice(V))
        ctx.render_slice(bent(), tile=(0, 0, 0, 0))
        ctx.render_slice(bent(), tile=(W, 0, 8, 8))
        ctx.render_slice(bent(), tile=(-20, -20, 20, 20))
        assert (_bits(ctx.read_backbuffer()) == _bits(before)).all()
        out = N.VkSliceSample()
        assert N.lib().vk_slice_probe(ctx.handle, C.byref(ok), 0, 0, None) == INVALID
        assert N.lib().vk_slice_probe(ctx.handle, None, 0, 0, C.byref(out)) == INVALID
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, layout)
        try:
            before = ctx.read_backbuffer().copy()
            code, msg = _code(V, lambda: ctx.render_slice(_slice(V)))
            assert code == UNSUPPORTED and "slice" in msg, layout
            code, msg = _code(V, lambda: ctx.slice_probe(_slice(V), 1, 1))
            assert code == UNSUPPORTED and "slice" in msg, layout
            assert (_bits(ctx.read_backbuffer()) == _bits(before)).all()
        finally:
            ctx.close()
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        code, msg = _code(V, lambda: ctx.render_slice(_slice(V)))
        assert code == UNSUPPORTED and "slice" in msg
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        code, msg = _code(V, lambda: ctx.render_slice(_slice(V)))
        assert code == INVALID and "no volume" in msg
    finally:
        ctx.close()
    h = C.c_void_p()  # no backbuffer
    assert N.lib().vk_ctx_create(0, C.byref(h)) == 0
    try:
        s = _slice(V)
        assert N.lib().vk_render_slice(h, C.byref(s), 0, 0, 8, 8, 0) == INVALID
        assert N.lib().vk_slice_probe(h, C.byref(s), 0, 0, C.byref(N.VkSliceSample())) == INVALID
    finally:
        N.lib().vk_ctx_destroy(h)


def test_reshaping_with_slice_passes_does_not_leak_device_memory(V, vol):  # noqa: F811
    import torch

    s = _slice(V, 2, "mean")

    def cycle(ctx, i):
        k = 1 + i % 4
        ctx.frames_in_flight(k)
        ctx.resize_backbuffer(W + 64 * (i % 3), H + 40 * (i % 2))
        for _ in range(k + 1):
            f = ctx.frame_begin()
            ctx.render_slice(s, values=True)
            ctx.frame_end()
        ctx.frame_wait(f)
        ctx.slice_probe(s, 3, 3)

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    ctx = _ctx(V, vol)
    try:
        for i in range(12):  # every shape once: the allocator's pools are warm after this
            cycle(ctx, i)
        before = free_bytes()
        for i in range(40):
            cycle(ctx, i)
        after = free_bytes()
        assert before - after < (8 << 20), f"{(before - after) / 2**20:.1f} MiB of device memory lost over 40 reshapes"
    finally:
        ctx.close()
