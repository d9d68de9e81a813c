"""Gradient lighting of the table march (vk_set_lighting) on the MI355X: frames against the C restatement of the lit march
(tests/lit_restatement.c), exact skipping, identity lighting, the axes and world scaling on a ball, the other entry points, the refusals, the
modes that ignore lighting, the C++ host, and device memory over set / reset cycles."""
import ctypes as C

import numpy as np
import pytest

from gpu_helpers import V, _synced  # noqa: F401
from lit_helpers import build_restatement, light_vector, restate, solid_table, sphere_u8
from test_frames_gpu import _centred, _shot
from tf_helpers import band_pass_table, zero_band_table

pytestmark = pytest.mark.gpu

N256 = 256
HEAD = dict(direction="headlight", ambient=0.25, diffuse=0.75, specular=0.4, shininess=24.0)
WORLD = dict(direction=(0.4, -0.8, 0.45), ambient=0.1, diffuse=0.9, specular=0.6, shininess=64.0)
IDENTITY = dict(direction=(0.0, 1.0, 0.0), ambient=1.0, diffuse=0.0, specular=0.0, shininess=1.0)
MAX_ERR = {}  # the largest colour error against the restatement, per case (printed at the end of the frames test)


@pytest.fixture(scope="module")
def L(O, tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("lit_restatement_gpu"), O)


@pytest.fixture(scope="module")
def vols(O):
    standin = O.volume_standin_u8(N256)
    return {"standin": standin, "fog16": O.volume_fog_f16(128, dense_core=True),
            "noncubic": np.ascontiguousarray(standin[40:200, 16:240, 64:160])}  # (nz, ny, nx) = (160, 224, 96)


def _cam(V, W, H, k=0):
    return V.Camera(1.0 + 0.1 * k, 0.5 - 0.1 * k, 1.0 + 0.4 * k, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix()


def _render(V, ctx, cam, flags=0, dt=1.0, tile=None):
    ctx.set_camera_blob(cam)
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=dt, flags=flags | V.RENDER_COUNT).record(ctx, tile=tile)
    return ctx.read_backbuffer().copy(), ctx.read_steps().copy(), ctx.step_counts()


def _ctx(V, W, H, vol, layout, table=None, light=None, domain=(0.0, 1.0), out=None):
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F if out is None else out)
    if table is not None:
        ctx.set_transfer_function(table, domain)
    if light is not None:
        ctx.set_lighting(**light)
    V.VolumeTexture(ctx, vol, layout=layout)
    return ctx


def _lv(light):
    return light_vector(light["direction"], light["ambient"], light["diffuse"], light["specular"], light["shininess"])


FRAMES = [("160x90", 160, 90, None), ("1080p tile", 1920, 1080, (896, 476, 128, 128))]


@pytest.mark.parametrize("vname,layouts,domain", [("standin", ("LINEAR", "PACKED", "PACKED_PAIRS"), (0.0, 1.0)), ("fog16", ("LINEAR", "PACKED"), (0.0, 1.2)),
                                                  ("noncubic", ("LINEAR", "PACKED", "PACKED_PAIRS"), (0.0, 1.0))])
def test_frames_match_the_restatement(V, O, L, vols, vname, layouts, domain):
    vol = vols[vname]
    table = zero_band_table()
    for lname, light in (("headlight", HEAD), ("world light", WORLD)):
        for fname, W, H, tile in FRAMES:
            cam = _cam(V, W, H)
            ref, ref_steps = restate(L, O, cam, vol, W, H, table=table, domain=domain, light=_lv(light), tile=tile)
            ys, xs = (slice(None), slice(None)) if tile is None else (slice(tile[1], tile[1] + tile[3]), slice(tile[0], tile[0] + tile[2]))
            assert ref_steps[ys, xs].max() > 0
            for lay in layouts:
                ctx = _ctx(V, W, H, vol, getattr(V, "LAYOUT_" + lay), table, light, domain)
                try:
                    img, steps, _ = _render(V, ctx, cam, tile=tile)
                finally:
                    ctx.close()
                what = (vname, lname, fname, lay)
                assert (steps[ys, xs] == ref_steps[ys, xs]).all(), what
                err = float(np.abs(img[ys, xs, :3] - ref[ys, xs, :3]).max())
                MAX_ERR[what] = err
                assert err <= 1e-4, (what, err)
    print("\nlit frames vs restatement, largest colour error:", max(MAX_ERR.values()), max(MAX_ERR, key=MAX_ERR.get))


def test_skip_policies_are_bitwise_equal(V, vols):
    cam = _cam(V, 320, 180)
    policies = [0, V.RENDER_NO_SKIP, V.RENDER_FORCE_SKIP, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS]
    for vname, lay in (("standin", "PACKED"), ("standin", "PACKED_PAIRS"), ("fog16", "PACKED")):
        for table in (zero_band_table(), band_pass_table()):
            ctx = _ctx(V, 320, 180, vols[vname], getattr(V, "LAYOUT_" + lay), table)
            try:
                unlit = [_render(V, ctx, cam, flags=f) for f in policies]
                ctx.set_lighting(**WORLD)
                outs = [_render(V, ctx, cam, flags=f) for f in policies]
            finally:
                ctx.close()
            for (img, steps, _), (_, unlit_steps, _) in zip(outs, unlit):
                assert (img.view(np.uint32) == outs[0][0].view(np.uint32)).all(), (vname, lay)
                assert (steps == outs[0][1]).all() and (steps == unlit_steps).all(), (vname, lay)
            assert not (outs[0][0].view(np.uint32) == unlit[0][0].view(np.uint32)).all(), (vname, lay)  # (the lighting did something)


def test_identity_lighting_is_the_unlit_table(V, vols):
    cam = _cam(V, 240, 136, 1)
    for vname, layouts in (("standin", ("LINEAR", "PACKED", "PACKED_PAIRS")), ("fog16", ("LINEAR", "PACKED"))):
        for lay in layouts:
            ctx = _ctx(V, 240, 136, vols[vname], getattr(V, "LAYOUT_" + lay), zero_band_table())
            try:
                ref = _render(V, ctx, cam)
                for light in (IDENTITY, dict(IDENTITY, direction="headlight")):
                    ctx.set_lighting(**light)
                    got = _render(V, ctx, cam)
                    assert (got[0].view(np.uint32) == ref[0].view(np.uint32)).all() and (got[1] == ref[1]).all(), (vname, lay)
                ctx.set_lighting(None)
                got = _render(V, ctx, cam)
                assert (got[0].view(np.uint32) == ref[0].view(np.uint32)).all(), (vname, lay)
            finally:
                ctx.close()


@pytest.mark.parametrize("dims", [(128, 128, 128), (160, 96, 64)])
def test_ball_lit_along_the_view_and_across_it(V, dims):
    """A ball viewed along +z: with a headlight the centre of the disc faces the light and is brighter than the limb; with a light along x
    the limb (on both sides: the shading is two-sided) is brighter than the centre.  Holds for a non-cubic grid only if the gradient is
    scaled to world units."""
    W = H = 128
    cam = V.Camera(1.2, 0.0, 0.0, (0.5, 0.5, 0.5), 1.0).get_proj_view_matrix()  # eye (0.5, 0.5, -0.7): a disc ~44 pixels across
    vol = sphere_u8(*dims)
    shots = {}
    for name, direction in (("head", "headlight"), ("x", (1.0, 0.0, 0.0))):
        ctx = _ctx(V, W, H, vol, V.LAYOUT_AUTO, solid_table(), dict(direction=direction, ambient=0.05, diffuse=0.95, specular=0.0, shininess=1.0))
        try:
            shots[name] = _render(V, ctx, cam)
        finally:
            ctx.close()
    row = H // 2
    hit = np.nonzero(shots["head"][0][row, :, 0] > 0)[0]  # (the table is transparent outside the ball: the disc is what has colour)
    assert 32 < len(hit) < W - 8 and (shots["x"][0][row, :, 0] > 0).sum() == len(hit)
    # the disc's first hits: the ball's visible radius in pixels from the centre column, the limb three pixels inside its edge
    centre, left, right = (hit[0] + hit[-1]) // 2, hit[0] + 3, hit[-1] - 3
    head, xl = shots["head"][0][row, :, 0], shots["x"][0][row, :, 0]
    assert head[centre] > head[left] + 0.1 and head[centre] > head[right] + 0.1, (head[left], head[centre], head[right])
    assert xl[left] > xl[centre] + 0.1 and xl[right] > xl[centre] + 0.1, (xl[left], xl[centre], xl[right])


def test_other_entry_points_under_lighting(V, vols):
    import torch

    W, H = 320, 200
    table = zero_band_table()
    cams = [_cam(V, W, H, k) for k in range(4)]
    ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, table, HEAD)
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
        ctx.set_camera_blob(cams[2])
        pipe.record(ctx)
        whole = ctx.read_backbuffer().copy()
        ts = 32
        slots = V.partition_slots(W, H, ts, 1)
        gathered = _synced(torch.full((1, slots, ts, ts, 4), float("nan"), dtype=torch.float32, device="cuda"))
        pipe.record_partition(ctx, ts, 0, 1, gathered.data_ptr())
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        V.native.check(ctx.handle, V.native.lib().vk_untile(ctx.handle, gathered.data_ptr(), ts, 1, slots))
        assert (ctx.read_backbuffer().view(np.uint32) == whole.view(np.uint32)).all(), "partition"
        # fused present == render + vk_present: within one 8-bit step, equal at every texel centre
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
    # frames in flight at K = 4: the lighting changes between frames 1 and 2 (outside a frame) and inside frame 3 (between vk_frame_begin and
    # its render: lighting is host state taken at record time); each frame is the single-surface render under the lighting it was recorded with
    plan = [HEAD, HEAD, WORLD, None]
    ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, table, HEAD)
    try:
        ctx.frames_in_flight(4)
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
        ids = []
        for k in range(4):
            if k == 2:
                ctx.set_lighting(**WORLD)
            ctx.set_camera_blob(cams[k])
            fid = ctx.frame_begin()
            if k == 3:
                ctx.set_lighting(None)
            pipe.record(ctx)
            ctx.frame_end()
            ids.append(fid)
        got = [ctx.read_frame(f).copy() for f in ids]
    finally:
        ctx.close()
    for k, g in enumerate(got):
        ref_ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, table, plan[k])
        try:
            ref_ctx.set_camera_blob(cams[k])
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5).record(ref_ctx)
            ref = ref_ctx.read_backbuffer()
        finally:
            ref_ctx.close()
        assert (g.view(np.uint32) == ref.view(np.uint32)).all(), ("frames in flight", k)


def _setl(lib, ctx, direction, head, ka, kd, ks, n):
    from vokselis_amd import _native as N

    li = N.VkLighting()
    li.dir[0], li.dir[1], li.dir[2] = direction
    li.headlight, li.ambient, li.diffuse, li.specular, li.shininess = head, ka, kd, ks, n
    return lib.vk_set_lighting(ctx.handle, C.byref(li))


def test_refusals_leave_the_lighting_in_force(V, O, vols):
    from vokselis_amd import _native as N

    W, H = 160, 90
    cam = _cam(V, W, H)
    lib = N.lib()
    ctx = _ctx(V, W, H, vols["standin"], V.LAYOUT_PACKED_PAIRS, zero_band_table(), WORLD)
    try:
        ref = _render(V, ctx, cam)
        nan, inf = float("nan"), float("inf")
        bad = [_setl(lib, ctx, (0.0, 0.0, 0.0), 0, 0.3, 0.7, 0.2, 32.0),
               _setl(lib, ctx, (nan, 1.0, 0.0), 0, 0.3, 0.7, 0.2, 32.0),
               _setl(lib, ctx, (nan, 1.0, 0.0), 1, 0.3, 0.7, 0.2, 32.0),  # (ignored with a headlight, but still not finite)
               _setl(lib, ctx, (1.0, inf, 0.0), 0, 0.3, 0.7, 0.2, 32.0),
               _setl(lib, ctx, (1.0, 0.0, 0.0), 0, -0.01, 0.7, 0.2, 32.0),
               _setl(lib, ctx, (1.0, 0.0, 0.0), 0, 0.3, 16.5, 0.2, 32.0),
               _setl(lib, ctx, (1.0, 0.0, 0.0), 0, 0.3, 0.7, 17.0, 32.0),
               _setl(lib, ctx, (1.0, 0.0, 0.0), 0, 0.3, 0.7, nan, 32.0),
               _setl(lib, ctx, (1.0, 0.0, 0.0), 0, 0.3, 0.7, 0.2, 0.5),
               _setl(lib, ctx, (1.0, 0.0, 0.0), 0, 0.3, 0.7, 0.2, 1025.0),
               _setl(lib, ctx, (1.0, 0.0, 0.0), 0, 0.3, 0.7, 0.2, inf)]
        assert all(rc == -1 for rc in bad), bad  # VK_ERR_INVALID
        with pytest.raises(V.VokselisError):
            ctx.set_lighting((0.0, 0.0, 0.0))
        got = _render(V, ctx, cam)
        assert (got[0].view(np.uint32) == ref[0].view(np.uint32)).all() and (got[1] == ref[1]).all()
        # the bounds themselves are valid
        assert _setl(lib, ctx, (0.0, 0.0, 0.0), 1, 0.0, 16.0, 16.0, 1024.0) == 0 and _setl(lib, ctx, (1e-30, 0.0, 0.0), 0, 16.0, 0.0, 0.0, 1.0) == 0
        with pytest.raises(V.VokselisError) as e:
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, flags=V.RENDER_FAST_WALK | V.RENDER_FORCE_SKIP).record(ctx)
        assert e.value.code == -5
        # lighting without a table
        ctx.set_transfer_function(None)
        with pytest.raises(V.VokselisError) as e:
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)
        assert e.value.code == -5 and "table" in str(e.value)
        ctx.set_lighting(None)
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)
    finally:
        ctx.close()
    ctx = _ctx(V, W, H, O.volume_standin_u8(64), V.LAYOUT_STAGED, zero_band_table(), HEAD)
    try:
        ctx.set_camera_blob(cam)
        with pytest.raises(V.VokselisError) as e:
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR).record(ctx)
        assert e.value.code == -5
    finally:
        ctx.close()


def test_modes_that_ignore_lighting(V):
    W, H = 128, 72
    cam = _cam(V, W, H)
    xor, proc = [], []
    for lit in (False, True):
        ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
        try:
            if lit:
                ctx.set_lighting(**WORLD)  # (no table: only NAIVE renders would refuse)
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


def test_no_device_memory_lost_over_lighting_cycles(V, O):
    import torch

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    W, H = 96, 64
    vol = O.volume_standin_u8(64)
    cam = _cam(V, W, H)
    ctx = _ctx(V, W, H, vol, V.LAYOUT_PACKED_PAIRS, zero_band_table())
    try:
        def cycle(i):
            ctx.set_lighting(**(HEAD if i & 1 else WORLD))
            _render(V, ctx, cam)
            ctx.set_lighting(None)
            _render(V, ctx, cam)

        for i in range(6):
            cycle(i)
        before = free_bytes()
        for i in range(100):
            cycle(i)
        after = free_bytes()
        assert before - after < (8 << 20), f"{(before - after) / 2**20:.1f} MiB of device memory lost over 100 lighting cycles"
    finally:
        ctx.close()


def test_cpp_host_bonsai_with_lighting(V, tmp_path):
    """bonsai --tf FILE --headlight / --light X Y Z [--light-params KA KD KS N] presents the same bytes as the Python path with the same table
    and lighting."""
    import os
    import subprocess

    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(g.ROOT, "vokselis_amd", "_lib", "bonsai")
    W, H = 320, 180
    table = zero_band_table()
    tf = tmp_path / "table.f32"
    table.astype("<f4").tofile(tf)
    for args, light in ((["--headlight"], dict(direction="headlight")),
                        (["--light", "0.4", "-0.8", "0.45", "--light-params", "0.1", "0.9", "0.6", "64"], WORLD)):
        ppm = tmp_path / "bonsai.ppm"
        r = subprocess.run([exe, "--frames", "1", "--size", f"{W}x{H}", "--dt", "1.0", "--tf", str(tf), *args, "--ppm", str(ppm)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        hdr, data = ppm.read_bytes().split(b"\n255\n", 1)
        assert hdr == f"P6\n{W} {H}".encode()
        got = np.frombuffer(data, np.uint8).reshape(H, W, 3)
        ctx = V.Context(W, H, V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H), backbuffer=(W, H))
        try:
            ctx.set_transfer_function(table)
            ctx.set_lighting(**light)
            V.VolumeTexture.generate_standin(ctx)
            ctx.update()
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
            ctx.render()
            want = _shot(ctx)[..., :3]
            ctx.set_lighting(None)
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
            ctx.render()
            unlit = _shot(ctx)[..., :3]
        finally:
            ctx.close()
        assert (got == want).all() and want.max() > 30, args
        assert (want != unlit).any(), args
    r = subprocess.run([exe, "--frames", "1", "--headlight"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "table" in r.stderr  # lighting without a table: the library's refusal
