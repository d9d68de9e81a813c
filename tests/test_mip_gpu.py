"""The maximum-intensity projection (vk_set_projection) on the MI355X as state and through every submission path: no table is the
explicit grey ramp, the order of the two setters does not matter, reset restores the compositing frames, maps and empty fraction bit
for bit, the projection survives uploads, the refusals, lighting and the other modes, tiles / batches / partitions / frames in flight /
the group / the fused present / the C++ host, device memory over set / reset / upload cycles, and a sanity check on the C2 volume."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mip_helpers as MH
from gpu_helpers import V, _synced  # noqa: F401
from test_frames_gpu import _centred, _shot
from test_transfer_gpu import _cam, _empty_fraction, _render
from tf_helpers import band_pass_table, zero_band_table

pytestmark = pytest.mark.gpu

N256 = 256
WINDOW = (0.1, 0.9)


@pytest.fixture(scope="module")
def vols(O):
    return {"standin": O.volume_standin_u8(N256), "small": O.volume_standin_u8(64), "fog16": O.volume_fog_f16(96, dense_core=True)}


def _ctx(V, W, H, vol, layout, table=None, domain=(0.0, 1.0), proj="max", out=None):
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F if out is None else out)
    try:
        if table is not None:
            ctx.set_transfer_function(table, domain)
        ctx.set_projection(proj)
        V.VolumeTexture(ctx, vol, layout=layout)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _same(a, b):
    return (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1] == b[1]).all() and a[2] == b[2]


def test_python_surface(V, vols):
    assert (V.PROJ_COMPOSITE, V.PROJ_MAX) == (0, 1)
    ctx = V.Context(64, 64, backbuffer=(64, 64))
    try:
        assert ctx.projection is None
        ctx.set_projection("max")
        assert ctx.projection == "max"
        ctx.set_projection("composite")
        assert ctx.projection is None
        ctx.set_projection(V.PROJ_MAX)
        assert ctx.projection == "max"
        ctx.set_projection(None)
        assert ctx.projection is None
        with pytest.raises(ValueError):
            ctx.set_projection("min")
    finally:
        ctx.close()


def test_no_table_is_the_explicit_grey_ramp(V, vols):
    W, H = 320, 180
    cam = _cam(V, W, H)
    for vname, lays in (("standin", ("LINEAR", "PACKED", "PACKED_PAIRS")), ("fog16", ("LINEAR", "PACKED"))):
        for lay in lays:
            a = _ctx(V, W, H, vols[vname], getattr(V, "LAYOUT_" + lay))
            b = _ctx(V, W, H, vols[vname], getattr(V, "LAYOUT_" + lay), MH.GREY_RAMP, (0.0, 1.0))
            try:
                for flags in (0, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS, V.RENDER_NO_SKIP):
                    assert _same(_render(V, a, cam, flags=flags), _render(V, b, cam, flags=flags)), (vname, lay, flags)
                assert _empty_fraction(a) == _empty_fraction(b)
                img = _render(V, a, cam)[0]
                assert (img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all() and img[..., 0].max() > 0.3  # grey
            finally:
                a.close()
                b.close()


def test_setter_order_does_not_matter(V, vols):
    W, H = 320, 180
    cam = _cam(V, W, H, 1)
    table = zero_band_table()
    for lay in ("PACKED", "PACKED_PAIRS"):
        outs = []
        for order in range(4):
            ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
            try:
                if order == 0:    # both before the volume
                    ctx.set_projection("max"); ctx.set_transfer_function(table, WINDOW); V.VolumeTexture(ctx, vols["standin"], layout=getattr(V, "LAYOUT_" + lay))
                elif order == 1:
                    ctx.set_transfer_function(table, WINDOW); ctx.set_projection("max"); V.VolumeTexture(ctx, vols["standin"], layout=getattr(V, "LAYOUT_" + lay))
                elif order == 2:  # both after it
                    V.VolumeTexture(ctx, vols["standin"], layout=getattr(V, "LAYOUT_" + lay)); ctx.set_projection("max"); ctx.set_transfer_function(table, WINDOW)
                else:             # through another table and a reset of the projection
                    V.VolumeTexture(ctx, vols["standin"], layout=getattr(V, "LAYOUT_" + lay)); ctx.set_transfer_function(band_pass_table()); ctx.set_projection("max")
                    ctx.set_projection(None); ctx.set_transfer_function(table, WINDOW); ctx.set_projection("max")
                outs.append((_render(V, ctx, cam, flags=V.RENDER_PROBE_ALWAYS), _empty_fraction(ctx)))
            finally:
                ctx.close()
        for o, e in outs[1:]:
            assert _same(o, outs[0][0]) and e == outs[0][1], lay
        assert 0.0 < outs[0][1] < 1.0


def test_reset_restores_the_compositing_projection(V, vols):
    """set_projection(None) after MAX: the parent's frames, sampled steps and empty fraction, on the built-in transfer and under a table."""
    W, H = 320, 180
    cam = _cam(V, W, H, 1)
    for lay in ("PACKED", "PACKED_PAIRS"):
        for table in (None, band_pass_table()):
            fresh = _ctx(V, W, H, vols["standin"], getattr(V, "LAYOUT_" + lay), table, proj=None)
            used = _ctx(V, W, H, vols["standin"], getattr(V, "LAYOUT_" + lay), table, proj=None)
            try:
                ref = _render(V, fresh, cam, flags=V.RENDER_PROBE_ALWAYS)
                ef = _empty_fraction(fresh)
                used.set_projection("max")
                mip = _render(V, used, cam, flags=V.RENDER_PROBE_ALWAYS)
                assert not (mip[0].view(np.uint32) == ref[0].view(np.uint32)).all()
                used.set_projection(None)
                got = _render(V, used, cam, flags=V.RENDER_PROBE_ALWAYS)
                assert _same(got, ref) and _empty_fraction(used) == ef, (lay, table is None)
                for flags in (0, V.RENDER_FORCE_SKIP):
                    assert _same(_render(V, used, cam, flags=flags), _render(V, fresh, cam, flags=flags)), (lay, flags)
            finally:
                fresh.close()
                used.close()


def test_projection_persists_across_uploads(V, O, vols):
    W, H = 160, 90
    cam = _cam(V, W, H)
    ref_ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, zero_band_table(), WINDOW)
    try:
        ref = _render(V, ref_ctx, cam)
        ef = _empty_fraction(ref_ctx)
    finally:
        ref_ctx.close()
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        ctx.set_projection("max")  # before any volume
        ctx.set_transfer_function(zero_band_table(), WINDOW)
        V.VolumeTexture(ctx, O.volume_fog_u8(64), layout=V.LAYOUT_PACKED)
        V.VolumeTexture(ctx, vols["standin"], layout=V.LAYOUT_PACKED_PAIRS)
        assert ctx.projection == "max" and _same(_render(V, ctx, cam), ref) and _empty_fraction(ctx) == ef
        V.VolumeTexture.generate_standin(ctx, dims=(N256,) * 3, layout=V.LAYOUT_PACKED_PAIRS)
        assert ctx.projection == "max" and _same(_render(V, ctx, cam), ref) and _empty_fraction(ctx) == ef
    finally:
        ctx.close()


def test_refusals_leave_the_projection_in_force(V, O, vols):
    from vokselis_amd import _native as N

    W, H = 160, 90
    cam = _cam(V, W, H)
    lib = N.lib()
    ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, zero_band_table(), WINDOW)
    try:
        ref = _render(V, ctx, cam)
        ef = _empty_fraction(ctx)
        assert lib.vk_set_projection(ctx.handle, 2) == -1 and lib.vk_set_projection(ctx.handle, -1) == -1
        fid = ctx.frame_begin()
        rc = lib.vk_set_projection(ctx.handle, V.PROJ_COMPOSITE)
        ctx.frame_end()
        ctx.frame_wait(fid)
        assert rc == -1 and ctx.projection == "max"
        with pytest.raises(V.VokselisError) as e:
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, flags=V.RENDER_FAST_WALK | V.RENDER_FORCE_SKIP).record(ctx)
        assert e.value.code == -5 and "projection" in str(e.value)
        assert _same(_render(V, ctx, cam), ref) and _empty_fraction(ctx) == ef
        # and the other way round: refused while compositing, the compositing state stays
        ctx.set_projection(None)
        comp = _render(V, ctx, cam)
        assert lib.vk_set_projection(ctx.handle, 7) == -1 and ctx.projection is None
        assert _same(_render(V, ctx, cam), comp)
    finally:
        ctx.close()
    for lay in ("STAGED", "BRICKED", "QUADS"):
        for table in (None, zero_band_table()):
            ctx = _ctx(V, W, H, vols["small"], getattr(V, "LAYOUT_" + lay), proj=None)
            try:
                ctx.set_camera_blob(cam)
                V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)
                before = ctx.read_backbuffer().copy()
                ctx.set_projection("max")
                if table is not None:
                    ctx.set_transfer_function(table)
                with pytest.raises(V.VokselisError) as e:
                    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)
                assert e.value.code == -5 and "projection" in str(e.value), lay
                ctx.set_transfer_function(None)
                ctx.set_projection(None)
                V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)  # renders again after the reset, the frame it rendered before
                assert (ctx.read_backbuffer().view(np.uint32) == before.view(np.uint32)).all(), lay
            finally:
                ctx.close()


def test_lighting_changes_no_bit_under_max(V, vols):
    W, H = 320, 180
    cam = _cam(V, W, H)
    for table in (None, zero_band_table()):
        ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, table, WINDOW)
        try:
            ref = _render(V, ctx, cam)
            ctx.set_lighting("headlight", ambient=0.1, diffuse=2.0, specular=1.0, shininess=8.0)
            assert _same(_render(V, ctx, cam), ref), table is None  # (without a table the compositing projection refuses lighting; MAX renders)
            ctx.set_lighting((0.3, -1.0, 0.2))
            assert _same(_render(V, ctx, cam), ref), table is None
        finally:
            ctx.close()


def test_modes_that_ignore_the_projection(V, O):
    W, H = 128, 72
    cam = _cam(V, W, H)
    xor, proc = [], []
    for proj in (None, "max"):
        ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
        try:
            ctx.set_projection(proj)
            V.VolumeTexture.generate_xor(ctx, dims=(64, 64, 64))
            ctx.set_camera_blob(cam)
            V.RaycastPipeline(V.MODE_COMPUTE_NEAREST).record(ctx)
            xor.append(ctx.read_backbuffer().copy())
            V.RaycastPipeline(V.MODE_PROCEDURAL).record(ctx)
            proc.append(ctx.read_backbuffer().copy())
        finally:
            ctx.close()
    assert (xor[0].view(np.uint32) == xor[1].view(np.uint32)).all()
    assert (proc[0].view(np.uint32) == proc[1].view(np.uint32)).all()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_every_submission_path_gives_the_vk_render_frame(V, vols, fmt):
    import torch

    W, H, ts = 320, 200, 32
    out = V.OUT_RGBA32F if fmt == "f32" else V.OUT_RGBA16F
    tdt = torch.float32 if fmt == "f32" else torch.float16
    cams = [_cam(V, W, H, k) for k in range(6)]
    ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, zero_band_table(), WINDOW, out=out)
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
        for tile in ((0, 0, 192, 128), (192, 0, 128, 128), (0, 128, 192, 72), (192, 128, 128, 72)):
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
        for nr in (1, 2, 3):
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
        ctx.set_camera_blob(cams[5])
        slots = V.partition_slots(W, H, ts, 1)
        part = _synced(torch.full((1, slots, ts, ts, 4), float("nan"), dtype=tdt, device="cuda"))
        pipe.record_partition(ctx, ts, 0, 1, part.data_ptr())
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        V.native.check(ctx.handle, V.native.lib().vk_untile(ctx.handle, part.data_ptr(), ts, 1, slots))
        assert (ctx.read_backbuffer().view(np.uint8) == singles[5].view(np.uint8)).all()
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
        # the debug counters' flags leave the frame alone
        ctx.set_camera_blob(cams[0])
        for flags in (V.RENDER_COUNT | V.native.RENDER_DEBUG_TRIPS, V.RENDER_SAFE, V.RENDER_NO_SKIP, V.RENDER_FORCE_SKIP, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS):
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5, flags=flags).record(ctx)
            assert (ctx.read_backbuffer().view(np.uint8) == singles[0].view(np.uint8)).all(), flags
    finally:
        ctx.close()
    # frames in flight at K = 1..4; the projection changes between frames 2 and 3: each frame is the single render under its own state
    for K in (1, 2, 3, 4):
        ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, zero_band_table(), WINDOW, out=out)
        try:
            ctx.frames_in_flight(K)
            ids = []
            pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
            for k in range(5):
                ctx.set_camera_blob(cams[k])
                fid = ctx.frame_begin()
                pipe.record(ctx)
                ctx.frame_end()
                ids.append(fid)
            last = ctx.read_frame(ids[-1]).copy()
            assert (last.view(np.uint8) == singles[4].view(np.uint8)).all(), K
            if K > 1:
                assert (ctx.read_frame(ids[-2]).view(np.uint8) == singles[3].view(np.uint8)).all(), K
            ctx.set_projection(None)  # drains the ring
            ctx.set_camera_blob(cams[4])
            fid = ctx.frame_begin()
            pipe.record(ctx)
            ctx.frame_end()
            assert not (ctx.read_frame(fid).view(np.uint8) == singles[4].view(np.uint8)).all(), K
        finally:
            ctx.close()


def test_group_render_under_fake_rccl_honours_the_projection(V, O):
    import __graft_entry__ as g

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VK_RCCL_LIB=g.build_fake_rccl())
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "mip_shim_group_check.py")], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "mip_shim_group_check: OK" in r.stdout and r.stdout.count("under VK_PROJ_MAX") == 2, r.stdout


def test_cpp_host_bonsai_mip(V, tmp_path):
    """bonsai --mip [--tf FILE --tf-domain LO HI] writes the PPM the Python host presents under the same state."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(g.ROOT, "vokselis_amd", "_lib", "bonsai")
    W, H = 320, 180
    shots = []
    for table, domain in ((None, (0.0, 1.0)), (zero_band_table(64), (0.05, 0.9))):
        ppm = tmp_path / "bonsai.ppm"
        args = [exe, "--frames", "1", "--size", f"{W}x{H}", "--dt", "1.0", "--mip", "--ppm", str(ppm)]
        if table is not None:
            tf = tmp_path / "table.f32"
            table.astype("<f4").tofile(tf)
            args += ["--tf", str(tf), "--tf-domain", repr(domain[0]), repr(domain[1])]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        hdr, data = ppm.read_bytes().split(b"\n255\n", 1)
        assert hdr == f"P6\n{W} {H}".encode()
        got = np.frombuffer(data, np.uint8).reshape(H, W, 3)
        ctx = V.Context(W, H, V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H), backbuffer=(W, H))
        try:
            if table is not None:
                ctx.set_transfer_function(table, domain)
            ctx.set_projection("max")
            V.VolumeTexture.generate_standin(ctx)
            ctx.update()
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
            ctx.render()
            want = _shot(ctx)[..., :3]
        finally:
            ctx.close()
        assert (got == want).all() and want.max() > 30, domain
        shots.append(got)
    assert (shots[0] != shots[1]).any()
    # --mip with frames in flight and the fused present runs too
    r = subprocess.run([exe, "--frames", "6", "--size", f"{W}x{H}", "--mip", "--in-flight", "3", "--fuse-present", "--orbit"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_no_device_memory_lost_over_projection_cycles(V, O):
    import torch

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    W, H = 96, 64
    vol = O.volume_standin_u8(64)
    cam = _cam(V, W, H)
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        def cycle(i):
            ctx.set_projection("max")
            if i & 1:
                ctx.set_transfer_function(band_pass_table() if i & 2 else zero_band_table())
            V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED if i % 3 else V.LAYOUT_PACKED_PAIRS)
            _render(V, ctx, cam)
            ctx.set_projection(None)
            _render(V, ctx, cam)
            ctx.set_transfer_function(None)

        for i in range(8):
            cycle(i)
        before = free_bytes()
        for i in range(110):
            cycle(i)
        after = free_bytes()
        assert before - after < (8 << 20), f"{(before - after) / 2**20:.1f} MiB of device memory lost over 110 projection cycles"
    finally:
        ctx.close()


def test_c2_volume_max_frame_is_not_the_composite_frame(V, vols):
    """The C2 volume (256^3 stand-in), a crop of the 1080p frame: the MAX frame differs from the COMPOSITE frame, no pixel is brighter than
    T at the volume's maximum, and the rays that meet it show exactly that."""
    W, H = 1920, 1080
    tile = (704, 284, 512, 512)
    vol = vols["standin"]
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix()
    ctx = _ctx(V, W, H, vol, V.LAYOUT_PACKED_PAIRS, proj=None)
    try:
        comp = _render(V, ctx, cam, dt=0.5, tile=tile)[0]
        ctx.set_projection("max")
        mip = _render(V, ctx, cam, dt=0.5, tile=tile)[0]
        # a window that ends at 0.6 of the volume's maximum: every ray that meets denser material saturates and shows T's last entry exactly
        last = np.array([0.25, 0.5, 0.75], np.float32)
        ctx.set_transfer_function(np.array([[0, 0, 0, 1], [*last, 1]], np.float32), (0.0, 0.6 * float(vol.max()) / 255.0))
        sat = _render(V, ctx, cam, dt=0.5, tile=tile)[0]
    finally:
        ctx.close()
    ys, xs = slice(tile[1], tile[1] + tile[3]), slice(tile[0], tile[0] + tile[2])
    assert (mip[ys, xs].view(np.uint32) != comp[ys, xs].view(np.uint32)).any()
    # grey ramp: the pixel is srgb(U), U <= max(vol) / 255; a ray through the brightest voxels' neighbourhood comes close to it
    vmax = float(vol.max()) / 255.0
    top = 1.055 * vmax ** (1 / 2.4) - 0.055
    g = mip[ys, xs, 0]
    assert g.max() <= top + 1e-6 and g.max() >= 0.9 * top, (float(g.max()), top)
    assert (mip[ys, xs, 0] == mip[ys, xs, 1]).all() and (mip[ys, xs, 3] == 1.0).all()
    want = (1.055 * last.astype(np.float64) ** (1 / 2.4) - 0.055)
    brightest = sat[ys, xs, :3].reshape(-1, 3).max(axis=0)
    assert np.abs(brightest - want).max() <= 1e-6, (brightest, want)
    assert (np.abs(sat[ys, xs, :3] - want).max(axis=2) <= 1e-6).sum() > 1000  # the rays that meet the maximum: the tree's trunk and crown
