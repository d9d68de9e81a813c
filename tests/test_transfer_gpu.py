"""The runtime transfer function (vk_set_transfer_function) on the MI355X: frames against the C restatement of the march under a table
(tests/tf_restatement.c), exact skipping under the table's skip maps, reset, persistence across uploads, the other entry points, the
modes that ignore the table, the refusals, and device memory over set / reset / re-upload cycles."""
import ctypes as C

import numpy as np
import pytest

from gpu_helpers import V, _synced  # noqa: F401
from test_frames_gpu import _centred, _shot
from tf_helpers import band_pass_table, build_restatement, restate, single_entry_table, zero_band_table

pytestmark = pytest.mark.gpu

N256 = 256


@pytest.fixture(scope="module")
def L(O, tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("tf_restatement_gpu"), O)


@pytest.fixture(scope="module")
def vols(O):
    return {"standin": O.volume_standin_u8(N256), "fog16": O.volume_fog_f16(128, dense_core=True)}


def _cam(V, W, H, k=0):
    return V.Camera(1.0 + 0.1 * k, 0.5 - 0.1 * k, 1.0 + 0.4 * k, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix()


def _render(V, ctx, cam, flags=0, dt=1.0, tile=None):
    ctx.set_camera_blob(cam)
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=dt, flags=flags | V.RENDER_COUNT).record(ctx, tile=tile)
    return ctx.read_backbuffer().copy(), ctx.read_steps().copy(), ctx.step_counts()


def _empty_fraction(ctx):
    from vokselis_amd import _native as N

    f = C.c_double()
    N.check(ctx.handle, N.lib().vk_volume_empty_fraction(ctx.handle, C.byref(f)))
    return f.value


def _ctx(V, W, H, vol, layout, table=None, domain=(0.0, 1.0), out=None):
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F if out is None else out)
    if table is not None:
        ctx.set_transfer_function(table, domain)
    V.VolumeTexture(ctx, vol, layout=layout)
    return ctx


FRAMES = [("160x90", 160, 90, None), ("1080p tile", 1920, 1080, (896, 476, 128, 128))]


@pytest.mark.parametrize("vname,layouts", [("standin", ("LINEAR", "PACKED", "PACKED_PAIRS")), ("fog16", ("LINEAR", "PACKED"))])
def test_frames_match_the_restatement(V, O, L, vols, vname, layouts):
    vol = vols[vname]
    for tname, table, domain in (("zero band", zero_band_table(), (0.0, 1.0)), ("band pass", band_pass_table(), (0.0, 1.0) if vname == "standin" else (0.0, 1.2))):
        for fname, W, H, tile in FRAMES:
            cam = _cam(V, W, H)
            ref, ref_steps = restate(L, O, cam, vol, W, H, table=table, domain=domain, tile=tile)
            ys, xs = (slice(None), slice(None)) if tile is None else (slice(tile[1], tile[1] + tile[3]), slice(tile[0], tile[0] + tile[2]))
            for lay in layouts:
                ctx = _ctx(V, W, H, vol, getattr(V, "LAYOUT_" + lay), table, domain)
                try:
                    img, steps, _ = _render(V, ctx, cam, tile=None if tile is None else tile)
                finally:
                    ctx.close()
                what = (vname, tname, fname, lay)
                assert (steps[ys, xs] == ref_steps[ys, xs]).all(), what
                err = float(np.abs(img[ys, xs, :3] - ref[ys, xs, :3]).max())
                assert err <= 1e-5, (what, err)


def test_skipping_stays_exact(V, O, vols, golden_volumes):
    cam = _cam(V, 320, 180)
    policies = [0, V.RENDER_NO_SKIP, V.RENDER_FORCE_SKIP, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS]
    for vname, lay in (("standin", "PACKED"), ("standin", "PACKED_PAIRS"), ("fog16", "PACKED")):
        for table in (zero_band_table(), band_pass_table()):
            ctx = _ctx(V, 320, 180, vols[vname], getattr(V, "LAYOUT_" + lay), table)
            try:
                outs = [_render(V, ctx, cam, flags=f) for f in policies]
            finally:
                ctx.close()
            for img, steps, _ in outs[1:]:
                assert (img.view(np.uint32) == outs[0][0].view(np.uint32)).all(), (vname, lay)
                assert (steps == outs[0][1]).all(), (vname, lay)
    # the band pass leaves more cells empty and samples fewer steps than the built-in transfer
    ctx = _ctx(V, 320, 180, vols["standin"], V.LAYOUT_PACKED_PAIRS)
    try:
        _, _, (_, s_builtin) = _render(V, ctx, cam, flags=V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS)
        e_builtin = _empty_fraction(ctx)
        ctx.set_transfer_function(band_pass_table())
        _, _, (_, s_band) = _render(V, ctx, cam, flags=V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS)
        e_band = _empty_fraction(ctx)
    finally:
        ctx.close()
    assert s_band < s_builtin and e_band > e_builtin, (s_band, s_builtin, e_band, e_builtin)
    # a single non-zero entry on the adversarial volumes: skip == no skip
    cam32 = _cam(V, 96, 64)
    for vname, vol in golden_volumes.items():
        for j in (0, 25, 26, 40, 255):
            ctx = _ctx(V, 96, 64, vol, V.LAYOUT_PACKED, single_entry_table(j=j))
            try:
                a = _render(V, ctx, cam32, flags=V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS)
                b = _render(V, ctx, cam32, flags=V.RENDER_NO_SKIP)
            finally:
                ctx.close()
            assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1] == b[1]).all(), (vname, j)


def test_reset_is_a_context_that_never_had_a_table(V, vols):
    W, H = 320, 180
    cam = _cam(V, W, H, 1)
    for lay in ("PACKED", "PACKED_PAIRS"):
        fresh = _ctx(V, W, H, vols["standin"], getattr(V, "LAYOUT_" + lay))
        used = _ctx(V, W, H, vols["standin"], getattr(V, "LAYOUT_" + lay))
        try:
            ref = _render(V, fresh, cam, flags=V.RENDER_PROBE_ALWAYS)
            ef = _empty_fraction(fresh)
            used.set_transfer_function(band_pass_table())
            _render(V, used, cam)
            used.set_transfer_function(None)
            got = _render(V, used, cam, flags=V.RENDER_PROBE_ALWAYS)
            assert (got[0].view(np.uint32) == ref[0].view(np.uint32)).all() and (got[1] == ref[1]).all(), lay
            assert got[2][1] == ref[2][1] and _empty_fraction(used) == ef, lay
        finally:
            fresh.close()
            used.close()


def test_table_persists_across_uploads(V, O, L, vols):
    W, H = 160, 90
    cam = _cam(V, W, H)
    table = zero_band_table()
    ref, ref_steps = restate(L, O, cam, vols["standin"], W, H, table=table)
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        ctx.set_transfer_function(table)  # set before any volume
        V.VolumeTexture(ctx, O.volume_fog_u8(64), layout=V.LAYOUT_PACKED)
        V.VolumeTexture(ctx, vols["standin"], layout=V.LAYOUT_PACKED_PAIRS)
        img, steps, _ = _render(V, ctx, cam)
        assert (steps == ref_steps).all() and float(np.abs(img[..., :3] - ref[..., :3]).max()) <= 1e-5
        V.VolumeTexture.generate_standin(ctx, dims=(N256,) * 3, layout=V.LAYOUT_PACKED)
        img, steps, _ = _render(V, ctx, cam)
        assert (steps == ref_steps).all() and float(np.abs(img[..., :3] - ref[..., :3]).max()) <= 1e-5
    finally:
        ctx.close()


def test_other_entry_points_under_a_table(V, vols):
    import torch

    W, H = 320, 200
    table = zero_band_table()
    cams = [_cam(V, W, H, k) for k in range(8)]
    ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, table)
    try:
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
        singles = []
        for c in cams:
            ctx.set_camera_blob(c)
            pipe.record(ctx)
            singles.append(ctx.read_backbuffer().copy())
        frames = _synced(torch.zeros((len(cams), H, W, 4), dtype=torch.float32, device="cuda"))
        V.render_batch(ctx, pipe, cams, frames.data_ptr(), tile_size=32)
        ctx.sync()
        got = frames.cpu().numpy()
        for k in range(len(cams)):
            assert (got[k].view(np.uint32) == singles[k].view(np.uint32)).all(), ("batch", k)
        # a vk_render_partition of the whole frame, un-tiled: the single frame, bitwise
        for ts in (16, 32):
            ctx.set_camera_blob(cams[5])
            pipe.record(ctx)
            whole = ctx.read_backbuffer().copy()
            slots = V.partition_slots(W, H, ts, 1)
            gathered = _synced(torch.full((1, slots, ts, ts, 4), float("nan"), dtype=torch.float32, device="cuda"))
            pipe.record_partition(ctx, ts, 0, 1, gathered.data_ptr())
            V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
            V.native.check(ctx.handle, V.native.lib().vk_untile(ctx.handle, gathered.data_ptr(), ts, 1, slots))
            assert (ctx.read_backbuffer().view(np.uint32) == whole.view(np.uint32)).all(), ("partition", ts)
        # fused present == render + vk_present: the HDR backbuffer bitwise, the presented image equal at every texel centre, within one
        # 8-bit step elsewhere (the checks of test_frames_gpu.py::test_present_fused_equals_render_then_present)
        ctx.set_camera_blob(cams[1])
        pipe.record(ctx)
        ctx.render()
        bb0, two_pass = ctx.read_backbuffer().copy(), _shot(ctx)
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5, flags=V.RENDER_PRESENT).record(ctx)
        bb1, fused = ctx.read_backbuffer(), _shot(ctx)
        assert (bb1.view(np.uint8) == bb0.view(np.uint8)).all()
        centre = _centred(H)[:, None] & _centred(W)[None, :]
        d = np.abs(fused.astype(np.int32) - two_pass.astype(np.int32)).max(axis=2)
        assert (d[centre[:d.shape[0], :d.shape[1]]] == 0).all() and d.max() <= 1
        assert fused[..., :3].max() > 30
    finally:
        ctx.close()
    # frames in flight at K = 3: the table changes between frames 2 and 3; each frame is the single render under its own table
    other = band_pass_table()
    ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, table)
    try:
        ctx.frames_in_flight(3)
        ids = []
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
        for k in range(4):
            if k == 2:
                ctx.set_transfer_function(other)
            ctx.set_camera_blob(cams[k])
            fid = ctx.frame_begin()
            pipe.record(ctx)
            ctx.frame_end()
            ids.append(fid)
        got = [ctx.read_frame(f).copy() for f in ids[1:]]
    finally:
        ctx.close()
    for k, g in zip(range(1, 4), got):
        ref_ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, table if k < 2 else other)
        try:
            ref_ctx.set_camera_blob(cams[k])
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5).record(ref_ctx)
            ref = ref_ctx.read_backbuffer()
        finally:
            ref_ctx.close()
        assert (g.view(np.uint32) == ref.view(np.uint32)).all(), ("frames in flight", k)


def test_modes_that_ignore_the_table(V, O):
    W, H = 128, 72
    cam = _cam(V, W, H)
    xor = []
    proc = []
    for with_table in (False, True):
        ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
        try:
            if with_table:
                ctx.set_transfer_function(band_pass_table())
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


def test_refusals_leave_the_table_in_force(V, O, vols):
    from vokselis_amd import _native as N

    W, H = 160, 90
    cam = _cam(V, W, H)
    table = zero_band_table()
    ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, table)
    lib = N.lib()
    try:
        ref = _render(V, ctx, cam)
        ef = _empty_fraction(ctx)

        def setf(t, n, lo, hi):
            p = None if t is None else np.ascontiguousarray(t, np.float32).ctypes.data_as(C.POINTER(C.c_float))
            return lib.vk_set_transfer_function(ctx.handle, p, n, lo, hi)

        bad = []
        bad.append(setf(table[:1], 1, 0.0, 1.0))
        big = np.zeros((257, 4), np.float32)
        bad.append(setf(big, 257, 0.0, 1.0))
        t = table.copy(); t[7, 1] = np.nan
        bad.append(setf(t, 256, 0.0, 1.0))
        t = table.copy(); t[9, 0] = np.inf
        bad.append(setf(t, 256, 0.0, 1.0))
        t = table.copy(); t[9, 0] = -3e38; t[10, 0] = 3e38  # finite, but their difference is not: beyond VK_TF_MAX_COLOUR
        bad.append(setf(t, 256, 0.0, 1.0))
        t = table.copy(); t[3, 3] = 1.5
        bad.append(setf(t, 256, 0.0, 1.0))
        t = table.copy(); t[3, 3] = -0.1
        bad.append(setf(t, 256, 0.0, 1.0))
        bad.append(setf(table, 256, 1.0, 1.0))
        bad.append(setf(table, 256, 1.0, 0.0))
        bad.append(setf(table, 256, float("nan"), 1.0))
        bad.append(setf(table, 256, 0.0, float("inf")))
        assert all(rc == -1 for rc in bad), bad  # VK_ERR_INVALID
        fid = ctx.frame_begin()
        rc = setf(band_pass_table(), 256, 0.0, 1.0)
        ctx.frame_end()
        ctx.frame_wait(fid)
        assert rc == -1
        with pytest.raises(V.VokselisError) as e:
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, flags=V.RENDER_FAST_WALK | V.RENDER_FORCE_SKIP).record(ctx)
        assert e.value.code == -5
        got = _render(V, ctx, cam)
        assert (got[0].view(np.uint32) == ref[0].view(np.uint32)).all() and (got[1] == ref[1]).all() and _empty_fraction(ctx) == ef
    finally:
        ctx.close()
    for lay in ("STAGED", "BRICKED", "QUADS"):
        ctx = _ctx(V, W, H, O.volume_standin_u8(64), getattr(V, "LAYOUT_" + lay), table)
        try:
            ctx.set_camera_blob(cam)
            with pytest.raises(V.VokselisError) as e:
                V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)
            assert e.value.code == -5 and "transfer function" in str(e.value), lay
            ctx.set_transfer_function(None)
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)  # the built-in transfer renders these layouts as before
        finally:
            ctx.close()


def test_no_device_memory_lost_over_table_cycles(V, O):
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
            ctx.set_transfer_function(band_pass_table() if i & 1 else zero_band_table())
            V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED if i % 3 else V.LAYOUT_PACKED_PAIRS)
            _render(V, ctx, cam)
            ctx.set_transfer_function(None)
            _render(V, ctx, cam)

        for i in range(6):
            cycle(i)
        before = free_bytes()
        for i in range(50):
            cycle(i)
        after = free_bytes()
        assert before - after < (8 << 20), f"{(before - after) / 2**20:.1f} MiB of device memory lost over 50 table cycles"
    finally:
        ctx.close()


def test_cpp_host_bonsai_with_a_table(V, tmp_path):
    """bonsai --tf FILE [--tf-domain LO HI] (raw little-endian f32 RGBA rows) presents the same bytes as the Python path with the same
    table; a file that is not whole RGBA rows is an error exit."""
    import os
    import subprocess

    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(g.ROOT, "vokselis_amd", "_lib", "bonsai")
    W, H = 320, 180
    for table, domain in ((zero_band_table(), (0.0, 1.0)), (band_pass_table(n=64), (0.05, 0.9))):
        tf = tmp_path / "table.f32"
        table.astype("<f4").tofile(tf)
        ppm = tmp_path / "bonsai.ppm"
        args = [exe, "--frames", "1", "--size", f"{W}x{H}", "--dt", "1.0", "--tf", str(tf), "--ppm", str(ppm)]
        if domain != (0.0, 1.0):
            args += ["--tf-domain", repr(domain[0]), repr(domain[1])]
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        hdr, data = ppm.read_bytes().split(b"\n255\n", 1)
        assert hdr == f"P6\n{W} {H}".encode()
        got = np.frombuffer(data, np.uint8).reshape(H, W, 3)
        ctx = V.Context(W, H, V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H), backbuffer=(W, H))
        try:
            ctx.set_transfer_function(table, domain)
            V.VolumeTexture.generate_standin(ctx)
            ctx.update()
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
            ctx.render()
            want = _shot(ctx)[..., :3]
        finally:
            ctx.close()
        assert (got == want).all() and want.max() > 30, domain
    bad = tmp_path / "bad.f32"
    np.zeros(7, "<f4").tofile(bad)
    r = subprocess.run([exe, "--frames", "1", "--tf", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "RGBA rows" in r.stderr
