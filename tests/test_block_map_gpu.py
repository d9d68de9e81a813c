"""The block -> pixel map of the march kernels on the MI355X (vk_common.hpp: frame_view, map_pixel; vk_hostmath.hpp: the reciprocals of
block_map_make): every path that maps blocks -- whole-frame and compact batches, single-frame partitions, tile rectangles with an origin off
the screen, every kernel family -- against vk_render of the same camera, bit for bit, at the smallest shapes at which the map can go wrong:
images smaller than a tile, lanes outside the image, partial tiles, tile edges that are no power of two, frame counts around the frame runs'
eight, several ranks with a root skip.  Step counts are compared wherever the path writes them (single-frame launches).  The volume is 32^3
u8 fog with transparent 8^3 holes and the cameras stand back from it, so that skipping and culling both occur (asserted)."""
import numpy as np
import pytest

import np_partition_reference as NP
from gpu_helpers import V, _holes_volume  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (70, 45), (72, 40), (200, 136)]
TILES = [8, 24, 32, 64, 128]
FRAMES = [1, 2, 7, 8, 9, 17]
DEALS = [(2, 2), (3, 3), (5, 2)]  # (ranks, root_skip)
DT = 1.0


def _cameras(V, n, aspect):
    """Every frame its own camera, far enough out that the box leaves part of the screen empty."""
    return [V.Camera(1.6 + 0.04 * k, 0.5 - 0.04 * k, 1.0 + 0.25 * k, (0.5, 0.5, 0.5), aspect).get_proj_view_matrix() for k in range(n)]


@pytest.fixture(scope="module")
def volume():
    return _holes_volume(32, 0.4, seed=11, block=8)


def _ff(*shape):
    import torch

    t = torch.full(shape, -1, dtype=torch.int32, device="cuda")  # 0xFF bytes: what nobody writes shows
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _singles(V, ctx, mode, cams, flags=0):
    """vk_render of every camera: frames as bits [B][H][W][4] and step images [B][H][W]."""
    frames, steps = [], []
    for cam in cams:
        ctx.set_camera_blob(cam)
        V.RaycastPipeline(mode, dt_scale=DT, flags=flags | V.RENDER_COUNT).record(ctx)
        frames.append(NP.bits(ctx.read_backbuffer()).copy())
        steps.append(ctx.read_steps().copy())
    return np.stack(frames), np.stack(steps)


def _tables(V, ctx, ts, mode, cams):
    orders, n_active = [], []
    for cam in cams:
        ctx.set_camera_blob(cam)
        orders.append(ctx.partition_order(ts, mode).copy())
        n_active.append(ctx.partition_active(ts, 1, mode)[0])
    return orders, np.array(n_active)


def _check_batches(V, ctx, mode, cams, singles, W, H, ts, deals, flags=0):
    """Whole frames and compact buffers of one batch against the singles.  Returns the failures."""
    fails, B = [], len(cams)
    pipe = V.RaycastPipeline(mode, dt_scale=DT, flags=flags)
    frames = _ff(B, H, W, 4)
    V.render_batch(ctx, pipe, cams, frames.data_ptr(), tile_size=ts)
    ctx.sync()
    if not (_host(frames) == singles).all():
        fails.append(f"{W}x{H} ts {ts} frames {B}: whole-frame batch differs in {int((_host(frames) != singles).any(axis=-1).sum())} pixels")
    ctx.set_param("order_rays", 1 if B >= 4 else 3)  # vk_partition_order reports the order a batch of this size deals
    orders, n_active = _tables(V, ctx, ts, mode, cams)
    rec = NP.record_elems(ts, NP.WIRE_RGBA)
    for nr, k in deals:
        ctx.set_root_skip(k)
        cap = V.partition_slots(W, H, ts, nr, k)
        buf = _ff(nr, cap, B, rec)
        for r in range(nr):
            V.render_batch(ctx, pipe, cams, buf[r].data_ptr(), tile_size=ts, rank=r, nranks=nr, compact=True, slot_capacity=cap)
        ctx.sync()
        host = _host(buf)
        got = NP.untile(host, W, H, ts, orders, n_active, k, NP.WIRE_RGBA)
        if not (got == singles).all():
            fails.append(f"{W}x{H} ts {ts} frames {B} ranks {nr} root_skip {k}: un-tiled compact batch differs in {int((got != singles).any(axis=-1).sum())} pixels")
        if B > 2:
            continue
        want = NP.encode(singles, ts, orders, n_active, nr, k, NP.WIRE_RGBA, cap)  # ... and nothing else was written
        if not (host == want).all():
            fails.append(f"{W}x{H} ts {ts} frames {B} ranks {nr} root_skip {k}: {int((host != want).sum())} elements of the ranks' buffers are not the reference's records")
    ctx.set_root_skip(0)
    return fails


def _check_partition(V, ctx, mode, cam, single, steps, W, H, ts, nr, k, flags=0, other=None):
    """vk_render_partition of one frame, every rank, with step counts: the un-tiled frame and the steps of the active tiles' pixels.  The step
    image starts as ANOTHER camera's (`other`: a camera and its step image), so a block that writes no count shows as much as one that writes a wrong one."""
    fails = []
    ctx.set_param("order_rays", 3)
    ctx.set_camera_blob(cam)
    ctx.set_root_skip(k)
    orders, n_active = _tables(V, ctx, ts, mode, [cam])
    cap = V.partition_slots(W, H, ts, nr, k)
    buf = _ff(nr, cap, 1, NP.record_elems(ts, NP.WIRE_RGBA))
    ctx.set_camera_blob(other[0])
    V.RaycastPipeline(mode, dt_scale=DT, flags=flags | V.RENDER_COUNT).record(ctx)  # the step image holds the other camera's counts
    ctx.set_camera_blob(cam)
    pipe = V.RaycastPipeline(mode, dt_scale=DT, flags=flags | V.RENDER_COUNT)
    for r in range(nr):
        pipe.record_partition(ctx, ts, r, nr, buf[r].data_ptr())
    ctx.sync()
    got = NP.untile(_host(buf), W, H, ts, orders, n_active, k, NP.WIRE_RGBA)[0]
    if not (got == single).all():
        fails.append(f"{W}x{H} ts {ts} ranks {nr} root_skip {k}: un-tiled partition differs in {int((got != single).any(axis=-1).sum())} pixels")
    tx, ty = NP.tiles_xy(W, H, ts)
    active = NP.tile_pixels(NP.active_masks(orders, n_active, tx * ty), W, H, ts)[0]
    got_steps = ctx.read_steps()
    if (W, H) != SIZES[0] and not (other[1][active] != steps[active]).any():
        fails.append(f"{W}x{H} ts {ts}: the two cameras' step images agree on every active pixel: a missing write would not show")
    if not (got_steps[active] == steps[active]).all():
        fails.append(f"{W}x{H} ts {ts} ranks {nr} root_skip {k}: {int((got_steps[active] != steps[active]).sum())} step counts of the partition differ")
    if steps[~active].any():
        fails.append(f"{W}x{H} ts {ts}: vk_render counts steps in a tile the order calls inactive")
    ctx.set_root_skip(0)
    return fails


@pytest.mark.parametrize("W,H", SIZES)
def test_block_map_built_in_march(V, volume, W, H):
    """The built-in skip kernel: every tile edge x every frame count, whole frames and compact output of 1, 2, 3 and 5 ranks; single-frame
    partitions with step counts."""
    mode = V.MODE_NAIVE_TRILINEAR
    cams = _cameras(V, max(FRAMES), W / H)
    flags = V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    fails = []
    try:
        V.VolumeTexture(ctx, volume, layout=V.LAYOUT_PACKED_PAIRS)
        ctx.reset_step_counts()
        singles, steps = _singles(V, ctx, mode, cams, flags)
        if (W, H) == SIZES[-1]:
            s_ref, s_sampled = ctx.step_counts()
            assert (steps[0] == 0).any() and (steps[0] != 0).any(), "the cameras cull nothing, or everything"
            assert (singles[..., :3] != 0).any() and 0 < s_sampled < s_ref, "nothing is skipped"
        for i, ts in enumerate(TILES):
            for j, B in enumerate(FRAMES):
                deals = [(1, 0), DEALS[(i + j) % 3]] + ([DEALS[(i + j + 1) % 3]] if B in (7, 9) else [])
                fails += _check_batches(V, ctx, mode, cams[:B], singles[:B], W, H, ts, deals, flags)
            for nr, k in [(1, 0)] + DEALS + ([(2, 0xFFFFFFFF)] if ts == 24 else []):  # (a root_skip no round reaches: the plain deal)
                fails += _check_partition(V, ctx, mode, cams[i], singles[i], steps[i], W, H, ts, nr, k, flags, other=(cams[i + 6], steps[i + 6]))
    finally:
        ctx.close()
    for f in fails[:30]:
        print("FAIL", f)
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"


def test_block_map_tile_origin_off_screen(V, volume):
    """Tile rectangles from a negative origin compose to the frame, bits and step counts: the blocks' corners are off the screen."""
    W, H = 70, 45
    cam = _cameras(V, 1, W / H)[0]
    flags = V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS | V.RENDER_COUNT
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, volume, layout=V.LAYOUT_PACKED_PAIRS)
        ctx.set_camera_blob(cam)
        pipe = V.RaycastPipeline(dt_scale=DT, flags=flags)
        pipe.record(ctx)
        want, want_steps = NP.bits(ctx.read_backbuffer()).copy(), ctx.read_steps().copy()
        # the step image starts as another camera's, the backbuffer cleared: a block that writes nothing shows in both
        ctx.set_camera_blob(_cameras(V, 7, W / H)[6])
        pipe.record(ctx)
        assert (ctx.read_steps() != want_steps).any()
        ctx.set_camera_blob(cam)
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        for ty in range(-16, H + 16, 40):
            for tx in range(-16, W + 16, 40):
                pipe.record(ctx, (tx, ty, 40, 40))
        pipe.record(ctx, (W + 5, 3, 40, 40))  # wholly off the screen: dropped
        assert (NP.bits(ctx.read_backbuffer()) == want).all() and (ctx.read_steps() == want_steps).all()
    finally:
        ctx.close()


def _table():
    from vokselis_amd.context import transfer_table

    return transfer_table([(0.0, 0, 0, 0, 0), (0.06, 0, 0, 0, 0), (0.1, 1.0, 0.5, 0.2, 0.3), (1.0, 1.0, 1.0, 1.0, 0.8)], 64)


FAMILIES = ["skip", "no-skip", "table", "lit", "max", "iso", "compute records", "staged"]


@pytest.mark.parametrize("family", FAMILIES)
def test_block_map_every_family(V, volume, family):
    """One case per kernel family that shares the map, 72 x 40 with 24-pixel tiles: a batch of three frames, whole and compact over two ranks
    with a root skip, and a single-frame partition with step counts."""
    W, H, ts = 72, 40, 24
    mode, flags, layout = V.MODE_NAIVE_TRILINEAR, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS, V.LAYOUT_PACKED_PAIRS
    if family == "no-skip":
        flags = V.RENDER_NO_SKIP
    elif family == "staged":
        layout = V.LAYOUT_STAGED
    elif family == "compute records":
        mode, flags = V.MODE_COMPUTE_NEAREST, 0
    cams = _cameras(V, 3, W / H)
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        if family == "compute records":
            V.VolumeTexture.generate_xor(ctx, (32, 32, 32), 0.0)
        else:
            V.VolumeTexture(ctx, volume, layout=layout)
        if family in ("table", "lit", "max"):
            ctx.set_transfer_function(_table())
        if family == "lit":
            ctx.set_lighting((0.3, 0.8, 0.5))
        if family == "max":
            ctx.set_projection("max")
        if family == "iso":
            ctx.set_isosurface(0.12, (0.9, 0.7, 0.4), 4)
            ctx.set_lighting("headlight")
        singles, steps = _singles(V, ctx, mode, cams, flags)
        assert (singles[..., :3] != 0).any(), "the frames are empty"
        fails = _check_batches(V, ctx, mode, cams, singles, W, H, ts, [(1, 0), (2, 2)], flags)
        fails += _check_partition(V, ctx, mode, cams[1], singles[1], steps[1], W, H, ts, 3, 3, flags, other=(cams[2], steps[2]))
    finally:
        ctx.close()
    for f in fails:
        print("FAIL", f)
    assert not fails, f"{family}: {len(fails)} mismatches; first: {fails[0]}"
