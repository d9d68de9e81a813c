"""First-hit isosurface rendering (vk_set_isosurface) on the MI355X as state and through every submission path: the Python round trip,
the order of the three setters does not matter, reset restores the composite, table and MAX states bit for bit, the state survives
uploads, the refusals, lighting and the other modes, tiles / batches / partitions / frames in flight / the group / the fused present /
the C++ host, device memory over set / reset cycles, and a sanity check on the C2 volume."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_helpers import V, _synced  # noqa: F401
from test_frames_gpu import _centred, _shot
from test_transfer_gpu import _cam, _empty_fraction, _render
from tf_helpers import band_pass_table, zero_band_table

pytestmark = pytest.mark.gpu

ISO, COLOUR = 0.3, (0.9, 0.7, 0.4)
LIGHT = dict(direction="headlight", ambient=0.2, diffuse=0.8, specular=0.4, shininess=24.0)


@pytest.fixture(scope="module")
def vols(O):
    return {"small": O.volume_standin_u8(64), "fog16": O.volume_fog_f16(48, dense_core=True)}


def _ctx(V, W, H, vol, layout, iso=ISO, colour=COLOUR, refine=4, light=LIGHT, out=None):
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F if out is None else out)
    try:
        if iso is not None:
            ctx.set_isosurface(iso, colour, refine)
        if light is not None:
            ctx.set_lighting(**light)
        V.VolumeTexture(ctx, vol, layout=layout)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _same(a, b):
    return (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1] == b[1]).all() and a[2] == b[2]


def test_python_surface_round_trips(V):
    ctx = V.Context(64, 64, backbuffer=(64, 64))
    try:
        assert ctx.isosurface is None
        ctx.set_isosurface(0.25)
        assert ctx.isosurface == (0.25, (1.0, 1.0, 1.0), 4)
        ctx.set_isosurface(0.5, colour=(0.5, 0.25, 2.0), refine=16)
        assert ctx.isosurface == (0.5, (0.5, 0.25, 2.0), 16)
        assert ctx.projection is None
        ctx.set_projection("max")  # stored, and reported, while the isosurface is in force
        assert ctx.projection == "max" and ctx.isosurface == (0.5, (0.5, 0.25, 2.0), 16)
        ctx.set_isosurface(None)
        assert ctx.isosurface is None and ctx.projection == "max"
        ctx.set_isosurface(None)  # twice: nothing to do
        for bad in (dict(iso=float("nan")), dict(iso=float("inf")), dict(iso=0.5, colour=(float("nan"), 0, 0)), dict(iso=0.5, colour=(0, -2e30, 0)),
                    dict(iso=0.5, colour=(0, 0, float("inf")))):
            with pytest.raises(V.VokselisError) as e:
                ctx.set_isosurface(**bad)
            assert e.value.code == -1 and ctx.isosurface is None
        with pytest.raises(ValueError):
            ctx.set_isosurface(0.5, refine=17)
        s = V.VkIsosurface()
        s.iso, s.refine = 0.5, 17
        assert V.native.lib().vk_set_isosurface(ctx.handle, C.byref(s)) == -1 and ctx.isosurface is None
        ctx.set_isosurface(0.5, colour=(1e30, -1e30, 0.0), refine=0)  # the bounds themselves are accepted
        assert ctx.isosurface == (0.5, (float(np.float32(1e30)), float(np.float32(-1e30)), 0.0), 0)
    finally:
        ctx.close()


def test_setter_order_does_not_matter(V, vols):
    W, H = 160, 96
    cam = _cam(V, W, H, 1)
    table = zero_band_table()
    for lay in ("PACKED", "PACKED_PAIRS"):
        L = getattr(V, "LAYOUT_" + lay)
        outs = []
        for order in range(5):
            ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
            try:
                ctx.set_lighting(**LIGHT)
                if order == 0:    # all before the volume
                    ctx.set_isosurface(ISO, COLOUR); ctx.set_transfer_function(table, (0.1, 0.9)); ctx.set_projection("max"); V.VolumeTexture(ctx, vols["small"], layout=L)
                elif order == 1:
                    ctx.set_projection("max"); ctx.set_transfer_function(table, (0.1, 0.9)); V.VolumeTexture(ctx, vols["small"], layout=L); ctx.set_isosurface(ISO, COLOUR)
                elif order == 2:  # all after it, the isosurface first
                    V.VolumeTexture(ctx, vols["small"], layout=L); ctx.set_isosurface(ISO, COLOUR); ctx.set_projection("max"); ctx.set_transfer_function(table, (0.1, 0.9))
                elif order == 3:  # through another threshold, a reset and another table
                    V.VolumeTexture(ctx, vols["small"], layout=L); ctx.set_isosurface(0.6, (0.0, 1.0, 0.0), 1); ctx.set_transfer_function(band_pass_table())
                    ctx.set_isosurface(None); ctx.set_projection("max"); ctx.set_isosurface(ISO, COLOUR); ctx.set_transfer_function(table, (0.1, 0.9))
                else:             # the isosurface alone: table and projection change nothing under it
                    V.VolumeTexture(ctx, vols["small"], layout=L); ctx.set_isosurface(ISO, COLOUR)
                outs.append((_render(V, ctx, cam, flags=V.RENDER_PROBE_ALWAYS), _empty_fraction(ctx)))
            finally:
                ctx.close()
        for o, e in outs[1:]:
            assert _same(o, outs[0][0]) and e == outs[0][1], lay
        assert 0.0 < outs[0][1] < 1.0


def test_reset_restores_composite_table_and_max(V, vols):
    """set_isosurface(None): the frames, sampled steps and empty fraction of the state underneath, bit for bit."""
    W, H = 160, 96
    cam = _cam(V, W, H, 1)
    for lay in ("PACKED", "PACKED_PAIRS"):
        L = getattr(V, "LAYOUT_" + lay)
        for table, proj in ((None, None), (band_pass_table(), None), (zero_band_table(), "max"), (None, "max")):
            fresh, used = (V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F) for _ in range(2))
            try:
                for ctx in (fresh, used):
                    if table is not None:
                        ctx.set_transfer_function(table, (0.1, 0.9))
                    ctx.set_projection(proj)
                    V.VolumeTexture(ctx, vols["small"], layout=L)
                ref = _render(V, fresh, cam, flags=V.RENDER_PROBE_ALWAYS)
                ef = _empty_fraction(fresh)
                used.set_isosurface(ISO, COLOUR)
                iso = _render(V, used, cam, flags=V.RENDER_PROBE_ALWAYS)
                assert not (iso[0].view(np.uint32) == ref[0].view(np.uint32)).all() and _empty_fraction(used) != ef
                used.set_isosurface(None)
                assert _same(_render(V, used, cam, flags=V.RENDER_PROBE_ALWAYS), ref) and _empty_fraction(used) == ef, (lay, table is None, proj)
                for flags in (0, V.RENDER_FORCE_SKIP):
                    assert _same(_render(V, used, cam, flags=flags), _render(V, fresh, cam, flags=flags)), (lay, flags)
            finally:
                fresh.close()
                used.close()


def test_state_persists_across_uploads(V, O, vols):
    W, H = 160, 96
    cam = _cam(V, W, H)
    ref_ctx = _ctx(V, W, H, vols["small"], V.LAYOUT_PACKED_PAIRS)
    try:
        ref = _render(V, ref_ctx, cam)
        ef = _empty_fraction(ref_ctx)
    finally:
        ref_ctx.close()
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        ctx.set_isosurface(ISO, COLOUR)  # before any volume
        ctx.set_lighting(**LIGHT)
        V.VolumeTexture(ctx, O.volume_fog_u8(32), layout=V.LAYOUT_PACKED)
        V.VolumeTexture(ctx, vols["small"], layout=V.LAYOUT_PACKED_PAIRS)
        assert ctx.isosurface == (float(np.float32(ISO)), tuple(float(np.float32(v)) for v in COLOUR), 4)
        assert _same(_render(V, ctx, cam), ref) and _empty_fraction(ctx) == ef
        V.VolumeTexture.generate_standin(ctx, dims=(64,) * 3, layout=V.LAYOUT_PACKED_PAIRS)
        assert ctx.isosurface is not None and _empty_fraction(ctx) > 0.0
        gen = _render(V, ctx, cam)  # (the generated stand-in is another volume: its own frame, still an isosurface's)
        assert (gen[0][..., 3] == 1.0).all() and len(np.unique(gen[0][..., 0])) > 2
        ctx.set_lighting(None)
        assert len(np.unique(_render(V, ctx, cam)[0][..., 0])) == 2  # unlit: the surface's colour and the background
    finally:
        ctx.close()


def test_refusals_leave_the_state_in_force(V, vols):
    from vokselis_amd import _native as N

    W, H = 160, 96
    cam = _cam(V, W, H)
    lib = N.lib()
    ctx = _ctx(V, W, H, vols["small"], V.LAYOUT_PACKED_PAIRS)
    try:
        ref = _render(V, ctx, cam)
        ef = _empty_fraction(ctx)
        state = ctx.isosurface
        for bad in (dict(iso=float("nan")), dict(iso=0.5, colour=(0.0, 3e30, 0.0))):
            with pytest.raises(V.VokselisError):
                ctx.set_isosurface(**bad)
        s = N.VkIsosurface()
        s.iso, s.refine = 0.7, 4
        fid = ctx.frame_begin()
        rc_set, rc_off = lib.vk_set_isosurface(ctx.handle, C.byref(s)), lib.vk_set_isosurface(ctx.handle, None)
        ctx.frame_end()
        ctx.frame_wait(fid)
        assert rc_set == -1 and rc_off == -1 and ctx.isosurface == state
        with pytest.raises(V.VokselisError) as e:
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, flags=V.RENDER_FAST_WALK | V.RENDER_FORCE_SKIP).record(ctx)
        assert e.value.code == -5 and "isosurface" in str(e.value)
        assert _same(_render(V, ctx, cam), ref) and _empty_fraction(ctx) == ef and ctx.isosurface == state
        # and the other way round: refused while off, the composite state stays
        ctx.set_isosurface(None)
        ctx.set_lighting(None)
        comp = _render(V, ctx, cam)
        with pytest.raises(V.VokselisError):
            ctx.set_isosurface(float("-inf"))
        assert ctx.isosurface is None and _same(_render(V, ctx, cam), comp)
    finally:
        ctx.close()
    for lay in ("STAGED", "BRICKED", "QUADS"):
        ctx = _ctx(V, W, H, vols["small"], getattr(V, "LAYOUT_" + lay), iso=None, light=None)
        try:
            ctx.set_camera_blob(cam)
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)
            before = ctx.read_backbuffer().copy()
            ctx.set_isosurface(ISO, COLOUR)
            with pytest.raises(V.VokselisError) as e:
                V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)
            assert e.value.code == -5 and "isosurface" in str(e.value), lay
            assert ctx.isosurface is not None
            ctx.set_isosurface(None)
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)  # renders again after the reset, the frame it rendered before
            assert (ctx.read_backbuffer().view(np.uint32) == before.view(np.uint32)).all(), lay
        finally:
            ctx.close()


def test_lighting_changes_the_frame_and_no_step(V, vols):
    W, H = 160, 96
    cam = _cam(V, W, H)
    for vname, lay in (("small", "PACKED_PAIRS"), ("small", "LINEAR"), ("fog16", "PACKED")):
        ctx = _ctx(V, W, H, vols[vname], getattr(V, "LAYOUT_" + lay), light=None)
        try:
            unlit = _render(V, ctx, cam)
            hit = unlit[0][..., :3].max(axis=2) > 0
            assert hit.any() and not hit.all()
            ctx.set_lighting(**LIGHT)  # no table is set: compositing would refuse this, the isosurface renders
            lit = _render(V, ctx, cam)
            assert (lit[1] == unlit[1]).all() and lit[2] == unlit[2]
            assert (lit[0][hit] != unlit[0][hit]).any() and (lit[0][~hit] == unlit[0][~hit]).all()
            ctx.set_isosurface(ISO, COLOUR, 0)  # another refinement depth: other shading positions, the same steps and maps
            r0 = _render(V, ctx, cam)
            assert (r0[1] == unlit[1]).all() and r0[2] == unlit[2] and (r0[0] != lit[0]).any()
            ctx.set_lighting(None)
            assert _same(_render(V, ctx, cam), unlit)  # unlit, the depth is invisible
        finally:
            ctx.close()


def test_modes_that_ignore_the_isosurface(V):
    W, H = 128, 72
    cam = _cam(V, W, H)
    xor, proc = [], []
    for on in (False, True):
        ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
        try:
            if on:
                ctx.set_isosurface(ISO, COLOUR)
            V.VolumeTexture.generate_xor(ctx, dims=(64, 64, 64))
            ctx.set_camera_blob(cam)
            V.RaycastPipeline(V.MODE_COMPUTE_NEAREST).record(ctx)
            xor.append(ctx.read_backbuffer().copy())
            V.RaycastPipeline(V.MODE_PROCEDURAL).record(ctx)
            proc.append(ctx.read_backbuffer().copy())
        finally:
            ctx.close()
    assert (xor[0].view(np.uint32) == xor[1].view(np.uint32)).all() and xor[0][..., :3].max() > 0
    assert (proc[0].view(np.uint32) == proc[1].view(np.uint32)).all()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_every_submission_path_gives_the_vk_render_frame(V, vols, fmt):
    import torch

    W, H, ts = 200, 136, 32
    out = V.OUT_RGBA32F if fmt == "f32" else V.OUT_RGBA16F
    tdt = torch.float32 if fmt == "f32" else torch.float16
    cams = [_cam(V, W, H, k) for k in range(5)]
    ctx = _ctx(V, W, H, vols["small"], V.LAYOUT_PACKED_PAIRS, out=out)
    try:
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
        singles = []
        for c in cams:
            ctx.set_camera_blob(c)
            pipe.record(ctx)
            singles.append(ctx.read_backbuffer().copy())
        assert len({s.tobytes() for s in singles}) == len(cams)
        # tiles: the frame in four vk_render calls
        ctx.set_camera_blob(cams[2])
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        for tile in ((0, 0, 128, 64), (128, 0, 72, 64), (0, 64, 128, 72), (128, 64, 72, 72)):
            pipe.record(ctx, tile)
        assert (ctx.read_backbuffer().view(np.uint8) == singles[2].view(np.uint8)).all()
        # whole-frame batch
        B = len(cams)
        frames = _synced(torch.zeros((B, H, W, 4), dtype=tdt, device="cuda"))
        V.render_batch(ctx, pipe, cams, frames.data_ptr(), tile_size=ts)
        ctx.sync()
        got = frames.cpu().numpy()
        for k in range(B):
            assert (got[k].view(np.uint8) == singles[k].view(np.uint8)).all(), ("batch", k)
        # compact batches + vk_untile_batch for N ranks emulated on this GPU
        for nr in (1, 3):
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
                assert (got[k].view(np.uint8) == singles[k].view(np.uint8)).all(), ("ranks", nr, k)
        # vk_render_partition of the whole frame, un-tiled
        ctx.set_camera_blob(cams[4])
        slots = V.partition_slots(W, H, ts, 1)
        part = _synced(torch.full((1, slots, ts, ts, 4), float("nan"), dtype=tdt, device="cuda"))
        pipe.record_partition(ctx, ts, 0, 1, part.data_ptr())
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        V.native.check(ctx.handle, V.native.lib().vk_untile(ctx.handle, part.data_ptr(), ts, 1, slots))
        assert (ctx.read_backbuffer().view(np.uint8) == singles[4].view(np.uint8)).all()
        # fused present == render + vk_present under the rule of test_frames_gpu.py
        ctx.set_camera_blob(cams[1])
        pipe.record(ctx)
        ctx.render()
        bb0, two_pass = ctx.read_backbuffer().copy(), _shot(ctx)
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5, flags=V.RENDER_PRESENT).record(ctx)
        bb1, fused = ctx.read_backbuffer(), _shot(ctx)
        assert (bb1.view(np.uint8) == bb0.view(np.uint8)).all() and (bb0.view(np.uint8) == singles[1].view(np.uint8)).all()
        centre = _centred(H)[:, None] & _centred(W)[None, :]
        d = np.abs(fused.astype(np.int32) - two_pass.astype(np.int32)).max(axis=2)
        assert (d[centre[:d.shape[0], :d.shape[1]]] == 0).all() and d.max() <= 1
        assert fused[..., :3].max() > 30
    finally:
        ctx.close()
    # frames in flight at K = 4; the isosurface goes off between frames: each frame is the single render under its own state
    ctx = _ctx(V, W, H, vols["small"], V.LAYOUT_PACKED_PAIRS, out=out)
    try:
        ctx.frames_in_flight(4)
        ids = []
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
        for k in range(5):
            ctx.set_camera_blob(cams[k])
            fid = ctx.frame_begin()
            pipe.record(ctx)
            ctx.frame_end()
            ids.append(fid)
        assert (ctx.read_frame(ids[-1]).view(np.uint8) == singles[4].view(np.uint8)).all()
        assert (ctx.read_frame(ids[-2]).view(np.uint8) == singles[3].view(np.uint8)).all()
        ctx.set_lighting(None)
        ctx.set_isosurface(None)  # drains the ring
        ctx.set_camera_blob(cams[4])
        fid = ctx.frame_begin()
        pipe.record(ctx)
        ctx.frame_end()
        assert not (ctx.read_frame(fid).view(np.uint8) == singles[4].view(np.uint8)).all()
    finally:
        ctx.close()


def test_group_render_under_fake_rccl_honours_the_isosurface(V):
    import __graft_entry__ as g

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VK_RCCL_LIB=g.build_fake_rccl())
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "iso_shim_group_check.py")], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "iso_shim_group_check: OK" in r.stdout and r.stdout.count("under an isosurface") == 2, r.stdout


def test_cpp_host_bonsai_iso(V, tmp_path):
    """bonsai --iso V [--iso-colour R G B] [--iso-refine N] [--headlight] writes the PPM the Python host presents under the same state; --iso
    with --mip is refused."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(g.ROOT, "vokselis_amd", "_lib", "bonsai")
    W, H = 320, 180
    shots = []
    for lit in (False, True):
        ppm = tmp_path / "bonsai.ppm"
        args = [exe, "--frames", "1", "--size", f"{W}x{H}", "--dt", "1.0", "--iso", "0.25", "--iso-colour", "0.9", "0.7", "0.4", "--iso-refine", "6", "--ppm", str(ppm)]
        if lit:
            args += ["--headlight", "--light-params", "0.2", "0.8", "0.4", "24"]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        hdr, data = ppm.read_bytes().split(b"\n255\n", 1)
        assert hdr == f"P6\n{W} {H}".encode()
        got = np.frombuffer(data, np.uint8).reshape(H, W, 3)
        ctx = V.Context(W, H, V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H), backbuffer=(W, H))
        try:
            ctx.set_isosurface(0.25, (0.9, 0.7, 0.4), 6)
            if lit:
                ctx.set_lighting("headlight", ambient=0.2, diffuse=0.8, specular=0.4, shininess=24.0)
            V.VolumeTexture.generate_standin(ctx)
            ctx.update()
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
            ctx.render()
            want = _shot(ctx)[..., :3]
        finally:
            ctx.close()
        assert (got == want).all() and want.max() > 30, lit
        shots.append(got)
    assert (shots[0] != shots[1]).any()
    r = subprocess.run([exe, "--frames", "1", "--size", f"{W}x{H}", "--iso", "0.25", "--mip"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--iso" in r.stderr and "--mip" in r.stderr


def test_no_device_memory_lost_over_set_reset_cycles(V, O):
    import torch

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    W, H = 96, 64
    cam = _cam(V, W, H)
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, O.volume_standin_u8(32), layout=V.LAYOUT_PACKED_PAIRS)

        def cycle(i):
            ctx.set_isosurface(0.1 + 0.005 * (i % 100), COLOUR, i % 17)
            if i & 1:
                ctx.set_transfer_function(band_pass_table() if i & 2 else zero_band_table())
            if i % 5 == 0:
                _render(V, ctx, cam)
            ctx.set_isosurface(None)
            ctx.set_transfer_function(None)

        for i in range(8):
            cycle(i)
        before = free_bytes()
        for i in range(100):
            cycle(i)
        after = free_bytes()
        assert before - after < (8 << 20), f"{(before - after) / 2**20:.1f} MiB of device memory lost over 100 set / reset cycles"
    finally:
        ctx.close()


def test_c2_volume_iso_frame_is_neither_the_composite_nor_the_max_frame(V):
    """The C2 volume (256^3 stand-in), a crop of the 1080p frame at dt 0.5: three different frames; the unlit isosurface frame holds two
    colours only, the surface's and the background's."""
    W, H = 1920, 1080
    tile = (704, 284, 512, 512)
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix()
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture.generate_standin(ctx, layout=V.LAYOUT_PACKED_PAIRS)
        comp = _render(V, ctx, cam, dt=0.5, tile=tile)
        ctx.set_projection("max")
        mip = _render(V, ctx, cam, dt=0.5, tile=tile)
        ctx.set_isosurface(0.25, COLOUR)
        iso = _render(V, ctx, cam, dt=0.5, tile=tile)
        ctx.set_lighting(**LIGHT)
        lit = _render(V, ctx, cam, dt=0.5, tile=tile)
    finally:
        ctx.close()
    ys, xs = slice(tile[1], tile[1] + tile[3]), slice(tile[0], tile[0] + tile[2])
    crop = iso[0][ys, xs]
    assert (crop.view(np.uint32) != comp[0][ys, xs].view(np.uint32)).any() and (crop.view(np.uint32) != mip[0][ys, xs].view(np.uint32)).any()
    hit = crop[..., :3].max(axis=2) > 0
    assert 0.05 < hit.mean() < 0.95
    want = 1.055 * np.array(COLOUR, np.float64) ** (1 / 2.4) - 0.055
    assert np.abs(crop[hit][:, :3] - want).max() <= 1e-6 and (crop[~hit] == [0.0, 0.0, 0.0, 1.0]).all() and (crop[..., 3] == 1.0).all()
    # first hit: no ray marches further than under MAX, which runs every ray to its end or to saturation
    assert iso[2][0] < mip[2][0] and (iso[1] <= comp[1].max()).all()
    assert (lit[1] == iso[1]).all() and (lit[0][ys, xs][hit] != crop[hit]).any() and len(np.unique(lit[0][ys, xs][hit][:, 0])) > 100
