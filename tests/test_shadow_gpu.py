"""Light-direction shadows of the first-hit isosurface (vk_set_shadows) on the MI355X: the state and the submission
paths.  The arithmetic is held by tests/test_shadow_fuzz_gpu.py.

- Shadows take effect only under a lit isosurface whose light is not a headlight: set with a headlight, with lighting off or without an
  isosurface, the frame is the frame of shadows off bit for bit; set_shadows(None) restores the unshadowed frame bit for bit; strength 0 is
  the unshadowed frame within the lit bar.
- Host state like lighting: a value set between frame_begin and frame_end applies to the renders recorded after it; it survives an upload;
  vk_get_shadows round-trips; refused values leave the previous state in force.
- The shadowed frame through vk_render equals, bit for bit, the same frame tile by tile, through vk_render_batch (whole frames, and compact
  + vk_untile_batch) and through a ring of 4 frames in flight; with VK_RENDER_PRESENT the presented image is within the 1-LSB bar of
  tests/test_frames_gpu.py."""
import numpy as np
import pytest

from gpu_helpers import V, _synced  # noqa: F401
from test_frames_gpu import _centred, _shot
from test_table_fuzz_cpu import rel_err
from test_table_fuzz_gpu import TOL_LIT
from test_transfer_gpu import _cam

pytestmark = pytest.mark.gpu

ISO, COLOUR = 0.3, (0.9, 0.7, 0.4)
LIGHT = dict(direction=(1.0, 0.6, 0.4), ambient=0.2, diffuse=0.8, specular=0.4, shininess=24.0)
HEAD = dict(LIGHT, direction="headlight")
SHADOWS = (0.7, 2.0)
W, H, DT = 200, 136, 0.5


@pytest.fixture(scope="module")
def vol(O):
    return O.volume_standin_u8(64)


def _ctx(V, vol, layout=None, iso=True, light=LIGHT, shadows=SHADOWS, out=None):
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F if out is None else out)
    try:
        if iso:
            ctx.set_isosurface(ISO, COLOUR, 4)
        if light is not None:
            ctx.set_lighting(**light)
        if shadows is not None:
            ctx.set_shadows(*shadows)
        V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED_PAIRS if layout is None else layout)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _frame(V, ctx, cam, flags=0):
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
    ctx.set_camera_blob(cam)
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=DT, flags=flags).record(ctx)
    return ctx.read_backbuffer().copy()


def _eq(a, b):
    return bool((a.view(np.uint8) == b.view(np.uint8)).all())


def test_round_trip_and_refusals(V, vol):
    ctx = _ctx(V, vol, shadows=None)
    try:
        assert ctx.shadows is None
        ctx.set_shadows()
        assert ctx.shadows == (np.float32(0.7), 2.0)
        ctx.set_shadows(0.25, 8.0)
        assert ctx.shadows == (0.25, 8.0)
        for bad in ((float("nan"), 2.0), (0.5, float("inf")), (-0.01, 2.0), (1.01, 2.0), (0.5, -0.5), (0.5, 1024.5)):
            with pytest.raises(RuntimeError):
                ctx.set_shadows(*bad)
            assert ctx.shadows == (0.25, 8.0), bad
        for edge in ((0.0, 0.0), (1.0, 1024.0)):
            ctx.set_shadows(*edge)
            assert ctx.shadows == edge
        ctx.set_shadows(None)
        assert ctx.shadows is None
    finally:
        ctx.close()


def test_shadows_take_effect_only_under_a_lit_isosurface_with_a_directional_light(V, vol):
    cam = _cam(V, W, H, 1)
    for lay in (V.LAYOUT_PACKED_PAIRS, V.LAYOUT_PACKED, V.LAYOUT_LINEAR):
        ctx = _ctx(V, vol, lay, shadows=None)
        try:
            plain = _frame(V, ctx, cam)
            ctx.set_shadows(*SHADOWS)
            dark = _frame(V, ctx, cam)
            assert not _eq(dark, plain) and (dark[..., :3] <= plain[..., :3] + 1e-6).all() and (dark[..., 3] == 1.0).all()
            assert (dark[..., :3] < plain[..., :3] - 0.01).any(axis=2).mean() > 0.02  # a visible share of the frame darkens
            ctx.set_shadows(None)
            assert _eq(_frame(V, ctx, cam), plain)  # off: the unshadowed frame bit for bit
            ctx.set_shadows(0.0, SHADOWS[1])  # strength 0: k = 1 either way
            assert rel_err(_frame(V, ctx, cam)[..., :3], plain[..., :3]).max() <= TOL_LIT
            ctx.set_shadows(*SHADOWS)
            # a headlight: ignored
            ctx.set_lighting(**HEAD)
            head = _frame(V, ctx, cam)
            ctx.set_shadows(None)
            assert _eq(_frame(V, ctx, cam), head) and not _eq(head, plain)
            ctx.set_shadows(*SHADOWS)
            # lighting off: ignored
            ctx.set_lighting(None)
            unlit = _frame(V, ctx, cam)
            ctx.set_shadows(None)
            assert _eq(_frame(V, ctx, cam), unlit)
            ctx.set_shadows(*SHADOWS)
            # no isosurface (the built-in march): ignored
            ctx.set_isosurface(None)
            builtin = _frame(V, ctx, cam)
            ctx.set_shadows(None)
            assert _eq(_frame(V, ctx, cam), builtin) and not _eq(builtin, unlit)
            # ... and everything back: the shadowed frame again (the state was stored all along)
            ctx.set_shadows(*SHADOWS)
            ctx.set_isosurface(ISO, COLOUR, 4)
            ctx.set_lighting(**LIGHT)
            assert _eq(_frame(V, ctx, cam), dark)
        finally:
            ctx.close()


def test_state_survives_an_upload_and_applies_inside_a_frame(V, O, vol):
    cam = _cam(V, W, H, 2)
    ctx = _ctx(V, vol)
    try:
        dark = _frame(V, ctx, cam)
        V.VolumeTexture(ctx, O.volume_standin_u8(48), layout=V.LAYOUT_PACKED)
        assert ctx.shadows == (np.float32(0.7), 2.0)
        other = _frame(V, ctx, cam)
        V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED_PAIRS)
        assert _eq(_frame(V, ctx, cam), dark) and not _eq(other, dark)
        ctx.set_shadows(None)
        plain = _frame(V, ctx, cam)
        # between frame_begin and frame_end: the left part is recorded before the call, the right part after it; the split runs through the
        # columns the shadows change, so that both parts tell the two states apart
        cols = np.nonzero((dark != plain).any(axis=(0, 2)))[0]
        sx = int((cols.min() + cols.max()) // 2) // 8 * 8
        assert 0 < sx < W
        ctx.frames_in_flight(2)
        ctx.set_camera_blob(cam)
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=DT)
        fid = ctx.frame_begin()
        pipe.record(ctx, (0, 0, sx, H))
        ctx.set_shadows(*SHADOWS)
        pipe.record(ctx, (sx, 0, W - sx, H))
        ctx.frame_end()
        got = ctx.read_frame(fid)
        assert _eq(got[:, :sx], plain[:, :sx]) and _eq(got[:, sx:], dark[:, sx:])
        assert not _eq(plain[:, sx:], dark[:, sx:]) and not _eq(plain[:, :sx], dark[:, :sx])
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_every_submission_path_gives_the_vk_render_frame(V, vol, fmt):
    import torch

    ts = 32
    out = V.OUT_RGBA32F if fmt == "f32" else V.OUT_RGBA16F
    tdt = torch.float32 if fmt == "f32" else torch.float16
    cams = [_cam(V, W, H, k) for k in range(4)]
    ctx = _ctx(V, vol, out=out)
    try:
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=DT)
        singles = [_frame(V, ctx, c) for c in cams]
        assert len({s.tobytes() for s in singles}) == len(cams)
        ctx.set_shadows(None)
        assert not _eq(_frame(V, ctx, cams[2]), singles[2])  # the frames below are shadowed ones
        ctx.set_shadows(*SHADOWS)
        # tiles: the frame in four vk_render calls
        ctx.set_camera_blob(cams[2])
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        for tile in ((0, 0, 128, 64), (128, 0, 72, 64), (0, 64, 128, 72), (128, 64, 72, 72)):
            pipe.record(ctx, tile)
        assert _eq(ctx.read_backbuffer(), singles[2])
        # whole-frame batch
        B = len(cams)
        frames = _synced(torch.zeros((B, H, W, 4), dtype=tdt, device="cuda"))
        V.render_batch(ctx, pipe, cams, frames.data_ptr(), tile_size=ts)
        ctx.sync()
        got = frames.cpu().numpy()
        for k in range(B):
            assert _eq(got[k], singles[k]), ("batch", k)
        # compact batches + vk_untile_batch for 3 ranks emulated on this GPU
        nr = 3
        cap = V.partition_slots(W, H, ts, nr, 0)
        gathered = None
        for r in range(nr):
            buf = _synced(torch.zeros((cap, B, ts, ts, 4), dtype=tdt, device="cuda"))
            bid, act = V.render_batch(ctx, pipe, cams, buf.data_ptr(), tile_size=ts, rank=r, nranks=nr, compact=True, slot_capacity=cap)
            if gathered is None:
                gathered = _synced(torch.zeros((nr, act, B, ts, ts, 4), dtype=tdt, device="cuda"))
            ctx.sync()
            gathered[r] = buf[:act]
        frames.zero_()
        torch.cuda.synchronize()
        V.untile_batch(ctx, bid, gathered.data_ptr(), act, frames.data_ptr())
        ctx.sync()
        got = frames.cpu().numpy()
        for k in range(B):
            assert _eq(got[k], singles[k]), ("ranks", k)
        # fused present == render + vk_present under the rule of test_frames_gpu.py
        ctx.set_camera_blob(cams[1])
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        pipe.record(ctx)
        ctx.render()
        bb0, two_pass = ctx.read_backbuffer().copy(), _shot(ctx)
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=DT, flags=V.RENDER_PRESENT).record(ctx)
        bb1, fused = ctx.read_backbuffer(), _shot(ctx)
        assert _eq(bb1, bb0) and _eq(bb0, singles[1])
        centre = _centred(H)[:, None] & _centred(W)[None, :]
        d = np.abs(fused.astype(np.int32) - two_pass.astype(np.int32)).max(axis=2)
        assert (d[centre[:d.shape[0], :d.shape[1]]] == 0).all() and d.max() <= 1
        assert fused[..., :3].max() > 30
    finally:
        ctx.close()
    # a ring of 4 frames in flight
    ctx = _ctx(V, vol, out=out)
    try:
        ctx.frames_in_flight(4)
        ids = []
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=DT)
        for k in range(4):
            ctx.set_camera_blob(cams[k])
            fid = ctx.frame_begin()
            pipe.record(ctx)
            ctx.frame_end()
            ids.append(fid)
        for k in range(4):
            assert _eq(ctx.read_frame(ids[k]), singles[k]), ("ring", k)
    finally:
        ctx.close()
