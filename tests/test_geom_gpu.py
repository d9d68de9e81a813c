"""The geometry pass of the first-hit isosurface on the MI355X through its entry points (vk_render_geometry, vk_geometry_info,
vk_readback_geometry, vk_frame_geometry, vk_pick): picks against the full-frame pass, the hit mask against the
colour render, the state the pass must ignore, the clip box, frame slots, resizes, device memory over reshapes, and every refusal with
its status.  The records themselves are held bit for bit in tests/test_geom_fuzz_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import geom_helpers as GH
from gpu_helpers import V  # noqa: F401
from np_clip_reference import ray_hits_f64
from shadow_cases import two_balls

pytestmark = pytest.mark.gpu

W, H, DT, ISO, R = 128, 96, 0.5, 0.5, 4
CAM = (1.2, 0.3, -1.2, (0.5, 0.5, 0.5), W / H)  # from the +x side: the large ball in front
BOX = ((0.0, 0.0, 0.0), (0.7, 1.0, 1.0))  # cuts through the large ball
INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def vol():
    v = two_balls((48, 40, 44))
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return GH.build_restatement(tmp_path_factory.mktemp("geom_gpu"), O)


@pytest.fixture(scope="module")
def cam(O):
    return O.camera_blob(*CAM)


def _ctx(V, vol, cam, layout=None, iso=True):
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        if iso:
            ctx.set_isosurface(ISO, (1.0, 1.0, 1.0), R)
        if vol is not None:
            V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED if layout is None else layout)
        ctx.set_camera_blob(cam)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _records(ctx, **kw):
    ctx.render_geometry(DT, **kw)
    return np.stack(ctx.read_geometry(), axis=2)


def _code(V, fn):
    with pytest.raises(V.VokselisError) as e:
        fn()
    return e.value.code, str(e.value)


def test_pick_is_the_full_frame_record(V, vol, cam):  # noqa: F811
    ctx = _ctx(V, vol, cam)
    try:
        full = _records(ctx)
        hit = np.isfinite(full[:, :, 0, 3])
        assert 200 < hit.sum() < hit.size // 2
        # a pixel of a culled block: no ray within 16 pixels of its 8x8 block passes through the cube
        through = ray_hits_f64(cam, W, H)
        culled = next((x, y) for y in range(0, H, 8) for x in range(0, W, 8) if not through[max(y - 16, 0):y + 24, max(x - 16, 0):x + 24].any())
        ys, xs = np.nonzero(hit)
        inside = (int(xs[len(xs) // 2]), int(ys[len(ys) // 2]))
        miss = next((x, y) for y in range(H) for x in range(W) if through[y, x] and not hit[y, x])
        for x, y in (inside, miss, (0, 0), (W - 1, H - 1), (culled[0] + 3, culled[1] + 5), (int(xs[0]), int(ys[0])), (int(xs[-1]), int(ys[-1]))):
            h = V.native.VkHit()
            V.native.check(ctx.handle, V.native.lib().vk_pick(ctx.handle, x, y, DT, C.byref(h)))
            rec = np.array([*h.pos, h.t, *h.grad, h.value], np.float32).reshape(2, 4)
            assert (rec.view(np.uint32) == full[y, x].view(np.uint32)).all(), (x, y, rec, full[y, x])
            assert bool(h.hit) == bool(hit[y, x])
            p = ctx.pick(x, y, DT)
            assert (p is None) == (not hit[y, x])
            if p is not None:
                assert p.pos == tuple(full[y, x, 0, :3]) and p.t == full[y, x, 0, 3] and p.grad == tuple(full[y, x, 1, :3]) and p.value == full[y, x, 1, 3]
                g = np.array(p.grad, np.float64)
                assert p.normal is not None and np.allclose(p.normal, -g / np.linalg.norm(g), rtol=0, atol=1e-15)
                assert p.value >= ISO * 255.0
        # the picks wrote their pixels into the surface and nothing else
        again = np.stack(ctx.read_geometry(), axis=2)
        assert (again.view(np.uint32) == full.view(np.uint32)).all()
        assert _code(V, lambda: ctx.pick(W, 0))[0] == INVALID and _code(V, lambda: ctx.pick(0, H))[0] == INVALID
        info = ctx.geometry_info()
        assert (info["width"], info["height"]) == (W, H) and info["device_ptr"]
    finally:
        ctx.close()


def test_hit_mask_is_the_unlit_white_frames_non_black_pixels(V, vol, cam):  # noqa: F811
    ctx = _ctx(V, vol, cam)
    try:
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=DT).record(ctx)
        img = ctx.read_backbuffer().copy()
        full = _records(ctx)
        lit_up = (img[..., :3] != 0).any(axis=2)
        assert lit_up.sum() > 200 and (lit_up == np.isfinite(full[:, :, 0, 3])).all()
        assert (ctx.read_backbuffer().view(np.uint32) == img.view(np.uint32)).all()  # the pass leaves the backbuffer alone
    finally:
        ctx.close()


def test_lighting_shadows_table_and_projection_do_not_move_the_records(V, vol, cam):  # noqa: F811
    ctx = _ctx(V, vol, cam)
    try:
        base = _records(ctx)
        ctx.set_lighting(direction=(1.0, 0.3, 0.2), ambient=0.2, diffuse=0.8, specular=0.5, shininess=16.0)
        lit = _records(ctx)
        ctx.set_shadows(0.7, 2.0)
        shadowed = _records(ctx)
        table = np.linspace(0.0, 1.0, 16 * 4, dtype=np.float32).reshape(16, 4)
        ctx.set_transfer_function(table, (0.1, 0.9))
        ctx.set_projection(V.PROJ_MAX)
        ctx.set_isosurface(ISO, (0.1, 0.9, 0.4), R)  # another colour
        rest = _records(ctx)
        for other in (lit, shadowed, rest):
            assert (other.view(np.uint32) == base.view(np.uint32)).all()
    finally:
        ctx.close()


def test_clip_box_moves_t_as_the_restatement_says(V, O, lib, vol, cam):  # noqa: F811
    ctx = _ctx(V, vol, cam)
    try:
        free = _records(ctx)
        ctx.set_clip_box(*BOX)
        cut = _records(ctx)
        ctx.set_clip_box(None)
        again = _records(ctx)
    finally:
        ctx.close()
    want_free = GH.restate(lib, O, cam, vol, W, H, iso=ISO, refine=R, dt=DT)[0]
    want_cut, _, _, fl = GH.restate(lib, O, cam, vol, W, H, iso=ISO, refine=R, dt=DT, box=BOX)
    assert GH.same_bits(free, want_free).all() and GH.same_bits(cut, want_cut).all() and GH.same_bits(again, want_free).all()
    both = np.isfinite(free[:, :, 0, 3]) & np.isfinite(cut[:, :, 0, 3])
    assert (cut[:, :, 0, 3][both] > free[:, :, 0, 3][both]).sum() > 50  # the cut takes the front of the large ball away: its rays go on to the cut face or beyond
    assert ((fl & GH.FIRST) != 0).sum() > 20                            # ... and those that start inside it hit in their first iteration, on the cut face


def test_a_pass_inside_a_frame_lands_in_that_frames_slot(V, vol, cam, O):  # noqa: F811
    ctx = _ctx(V, vol, cam)
    try:
        ctx.frames_in_flight(4)
        assert _code(V, ctx.read_geometry)[0] == INVALID  # nothing has been rendered yet
        cams = [O.camera_blob(1.2, 0.3, 0.4 + 0.5 * k, (0.5, 0.5, 0.5), W / H) for k in range(4)]
        fids = []
        for k in range(4):
            ctx.set_camera_blob(cams[k])
            fids.append(ctx.frame_begin())
            ctx.render_geometry(DT)
            ctx.frame_end()
        got = [np.stack(ctx.frame_geometry(f), axis=2) for f in fids]
        ctx.frames_in_flight(1)
        for k in range(4):
            ctx.set_camera_blob(cams[k])
            assert (got[k].view(np.uint32) == _records(ctx).view(np.uint32)).all(), k
        assert not (got[0].view(np.uint32) == got[1].view(np.uint32)).all()
        # once a later frame has taken the slot, the frame's surface is gone
        ctx.frames_in_flight(4)
        ids = []
        for k in range(5):
            ids.append(ctx.frame_begin())
            ctx.render_geometry(DT)
            ctx.frame_end()
        code, msg = _code(V, lambda: ctx.frame_geometry(ids[0]))
        assert code == INVALID and "later frame" in msg
        assert np.isfinite(ctx.frame_geometry(ids[4])[0][..., 3]).any()
        # a frame whose slot never saw a geometry pass has no surface
        ctx.frames_in_flight(4)  # (a ring resize frees every slot's surface)
        f = ctx.frame_begin()
        ctx.frame_end()
        code, msg = _code(V, lambda: ctx.frame_geometry(f))
        assert code == INVALID and "no geometry pass" in msg
    finally:
        ctx.close()


def test_a_resize_drops_the_surface_until_the_next_pass(V, vol, cam):  # noqa: F811
    ctx = _ctx(V, vol, cam)
    try:
        assert _code(V, ctx.read_geometry)[0] == INVALID and _code(V, ctx.geometry_info)[0] == INVALID
        ctx.render_geometry(DT, tile=(8, 8, 16, 16))
        first = np.stack(ctx.read_geometry(), axis=2)
        m = np.zeros((H, W), bool)
        m[8:24, 8:24] = True
        assert GH.same_bits(first[~m], GH.MISS).all()  # the allocation's fill: the miss record everywhere the tile is not
        ctx.resize_backbuffer(W + 8, H - 8)
        assert _code(V, ctx.read_geometry)[0] == INVALID and _code(V, ctx.geometry_info)[0] == INVALID
        ctx.render_geometry(DT)
        pos_t, grad_x = ctx.read_geometry()
        assert pos_t.shape == (H - 8, W + 8, 4) and np.isfinite(pos_t[..., 3]).sum() > 200
        # a pitch larger than a row; a pitch smaller than one is refused
        rows = np.zeros((H - 8, (W + 8) * 8 + 16), np.float32)
        V.native.check(ctx.handle, V.native.lib().vk_readback_geometry(ctx.handle, rows.ctypes.data, rows.strides[0]))
        assert (rows[:, :(W + 8) * 8].reshape(H - 8, W + 8, 2, 4)[:, :, 0, :].view(np.uint32) == pos_t.view(np.uint32)).all() and (rows[:, (W + 8) * 8:] == 0).all()
        assert V.native.lib().vk_readback_geometry(ctx.handle, rows.ctypes.data, (W + 8) * 32 - 4) == INVALID
    finally:
        ctx.close()


def test_every_refusal_returns_its_status(V, vol, cam):  # noqa: F811
    ctx = _ctx(V, vol, cam)
    try:
        code, msg = _code(V, lambda: ctx.render_geometry(DT, flags=V.RENDER_FAST_WALK))
        assert code == UNSUPPORTED and "isosurface" in msg
        for flags in (V.RENDER_COUNT, V.RENDER_PRESENT, V.RENDER_PRESENT_ONLY, V.native.RENDER_DEBUG_TRIPS, 1 << 20):
            assert _code(V, lambda: ctx.render_geometry(DT, flags=flags))[0] == INVALID, flags
        for dt in (0.0, -1.0, float("nan"), float("inf")):
            assert _code(V, lambda: ctx.render_geometry(dt))[0] == INVALID, dt
        for flags in (V.RENDER_NO_SKIP, V.RENDER_SAFE, V.RENDER_FORCE_SKIP, V.RENDER_PROBE_ALWAYS, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS | V.RENDER_SAFE):
            ctx.render_geometry(DT, flags=flags)
        ctx.render_geometry(DT, tile=(0, 0, 0, 0))  # an empty tile is no error
        ctx.set_isosurface(None)
        code, msg = _code(V, lambda: ctx.render_geometry(DT))
        assert code == INVALID and "isosurface" in msg
        assert _code(V, lambda: ctx.pick(1, 1))[0] == INVALID
    finally:
        ctx.close()
    for layout in (V.LAYOUT_BRICKED, V.LAYOUT_QUADS, V.LAYOUT_STAGED):
        ctx = _ctx(V, vol, cam, layout=layout)
        try:
            code, msg = _code(V, lambda: ctx.render_geometry(DT))
            assert code == UNSUPPORTED and "isosurface" in msg, layout
        finally:
            ctx.close()
    ctx = _ctx(V, None, cam)  # no volume
    try:
        assert _code(V, lambda: ctx.render_geometry(DT))[0] == INVALID
    finally:
        ctx.close()


def test_reshaping_with_geometry_passes_does_not_leak_device_memory(V, vol, cam):  # noqa: F811
    import torch

    def cycle(ctx, i):
        k = 1 + i % 4
        ctx.frames_in_flight(k)
        ctx.resize_backbuffer(W + 64 * (i % 3), H + 40 * (i % 2))
        for _ in range(k + 1):
            f = ctx.frame_begin()
            ctx.render_geometry(DT)
            ctx.frame_end()
        ctx.frame_wait(f)
        ctx.pick(3, 3, DT)

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    ctx = _ctx(V, vol, cam)
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
