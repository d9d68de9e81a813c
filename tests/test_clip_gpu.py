"""The clip box (vk_set_clip_box) on the MI355X: the table, lit, MAX and isosurface kernels under a box over the shared
cases (tests/clip_cases.py), against the numpy references under the same box (tests/np_clip_reference.py).

For every case and every layout with such kernels (u8: LINEAR, PACKED, PACKED_PAIRS; f16: LINEAR, PACKED), through the Python API:
- per-pixel step counts equal the reference's, colour within the tolerance of the family's own GPU fuzz module, finite, alpha 1;
- every pixel whose reference ray misses the box is exactly (0, 0, 0, 1) with 0 steps (the tightened cull and the inactive tiles);
- the default policy, RENDER_NO_SKIP, RENDER_FORCE_SKIP | RENDER_PROBE_ALWAYS and RENDER_SAFE give bitwise-equal frames and steps; the
  production kernel gives the COUNT kernel's frame; RGBA16F output is the round-to-nearest-even of the RGBA32F frame (the cases marked
  `half`); pixels outside a tile stay untouched;
- no clipped case passes on an empty picture: at least 2 % of the tile's pixels step, and at least 2 % differ from the unclipped reference.
Then the unit box against no box, the state's rules, every other submission path against vk_render, and the active tiles."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_cases as CC
from gpu_helpers import V, _synced  # noqa: F401
from test_frames_gpu import _centred, _shot
from test_mip_fuzz_gpu import TOL as TOL_MIP
from test_table_fuzz_cpu import rel_err
from test_table_fuzz_gpu import TOL_LIT, TOL_UNLIT, _policies
from test_transfer_gpu import _cam, _empty_fraction

pytestmark = pytest.mark.gpu

U8_LAYOUTS, F16_LAYOUTS = ("LINEAR", "PACKED", "PACKED_PAIRS"), ("LINEAR", "PACKED")
TOL = {"table": TOL_UNLIT, "lit": TOL_LIT, "mip": TOL_MIP, "mip table": TOL_MIP, "iso": TOL_UNLIT, "iso lit": TOL_LIT}  # (the isosurface fuzz takes the table fuzz's two)
W, H = CC.W, CC.H


def _set_family(ctx, family, volume):
    if family in ("table", "lit", "mip table"):
        ctx.set_transfer_function(CC.table(), CC.DOMAIN[volume])
    if family == "lit":
        ctx.set_lighting(**CC.LIGHT)
    if family in ("mip", "mip table"):
        ctx.set_projection("max")
    if family in ("iso", "iso lit"):
        ctx.set_isosurface(CC.ISO[volume], (0.9, 0.7, 0.4), 4)
    if family == "iso lit":
        ctx.set_lighting(**CC.LIGHT_X)


def _context(V, O, family, volume, layout, box, out=None, size=(W, H)):
    ctx = V.Context(*size, backbuffer=size, out_format=V.OUT_RGBA32F if out is None else out)
    try:
        _set_family(ctx, family, volume)
        if box is not None:
            ctx.set_clip_box(*box)
        V.VolumeTexture(ctx, CC.volumes(O)[volume], layout=getattr(V, "LAYOUT_" + layout))
    except BaseException:
        ctx.close()
        raise
    return ctx


def _render(V, ctx, cam, dt, flags, tile=None):
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
    ctx.set_camera_blob(cam)
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=dt, flags=flags).record(ctx, tile)
    return ctx.read_backbuffer().copy(), (ctx.read_steps().copy() if flags & V.RENDER_COUNT else None)


def _layouts(O, volume):
    return F16_LAYOUTS if CC.volumes(O)[volume].dtype == np.float16 else U8_LAYOUTS


@pytest.mark.parametrize("family", CC.FAMILIES)
def test_clip_cases_against_the_references(V, O, family):  # noqa: F811
    fails, worst, runs, halves = [], (0.0, None), 0, 0
    cases = [c for c in CC.CASES if c.family == family]
    assert len(cases) >= 5
    for c in cases:
        cam = O.camera_blob(*CC.CAMERAS[c.camera])
        ref, ref_steps = CC.reference(O, c)
        ref0, ref_steps0 = CC.reference(O, c, box=None)
        m = CC.tile_mask(c)
        # the condition on the inputs: a clipped case must not pass on an empty picture
        hits = float((ref_steps[m] > 0).mean())
        differ = float(((ref[m] != ref0[m]).any(axis=-1) | (ref_steps[m] != ref_steps0[m])).mean())
        print(f"{c.name}: {hits:.1%} of the tile's pixels step, {differ:.1%} differ from the unclipped reference")
        if not c.miss:
            assert hits >= 0.02, (c, hits)
            if c.box != "unit":
                assert differ >= 0.02, (c, differ)
        missed = m & (ref_steps == 0) & (ref == 0).all(axis=-1)
        for lay in _layouts(O, c.volume):
            what = (c, lay)
            ctx = _context(V, O, c.family, c.volume, lay, CC.BOXES[c.box])
            try:
                frames = [(name, *_render(V, ctx, cam, c.dt, fl | V.RENDER_COUNT, c.tile)) for name, fl in _policies(V)]
                prod, _ = _render(V, ctx, cam, c.dt, 0, c.tile)
            finally:
                ctx.close()
            runs += 1
            _, img, steps = frames[0]
            if not (steps[m] == ref_steps[m]).all():
                fails.append((what, f"steps differ from the reference at {int((steps[m] != ref_steps[m]).sum())} pixels"))
            if not np.isfinite(img[m][..., :3]).all():
                fails.append((what, "non-finite output"))
            err = float(rel_err(img[m][..., :3], ref[m]).max())
            if err > TOL[family] or np.isnan(err):
                fails.append((what, f"colour error {err:.3g} > {TOL[family]}"))
            if err >= worst[0]:
                worst = (err, f"{c.name} / {lay}")
            if not (img[m][..., 3] == 1.0).all():
                fails.append((what, "alpha is not 1"))
            if not ((img[missed] == [0.0, 0.0, 0.0, 1.0]).all() and (steps[missed] == 0).all()):
                fails.append((what, "a pixel whose ray misses the box is not (0, 0, 0, 1) with 0 steps"))
            if c.tile is not None and not (img[~m] == [0.0, 0.0, 0.0, 1.0]).all():
                fails.append((what, "pixels outside the tile were written"))
            for name, other, osteps in frames[1:]:
                if not (other.view(np.uint32) == img.view(np.uint32)).all():
                    fails.append((what, f"policy '{name}' differs from '{frames[0][0]}' at {int((other.view(np.uint32) != img.view(np.uint32)).any(axis=2).sum())} pixels"))
                if not (osteps[m] == steps[m]).all():
                    fails.append((what, f"policy '{name}': steps differ"))
            if not (prod.view(np.uint32) == frames[1][1].view(np.uint32)).all():
                fails.append((what, "the production kernel differs from the COUNT kernel"))
            if c.half:
                ctx = _context(V, O, c.family, c.volume, lay, CC.BOXES[c.box], out=V.OUT_RGBA16F)
                try:
                    h, _ = _render(V, ctx, cam, c.dt, 0, c.tile)
                finally:
                    ctx.close()
                halves += 1
                if not (h.view(np.uint16) == prod.astype(np.float16).view(np.uint16)).all():
                    fails.append((what, "RGBA16F output is not the RNE of the RGBA32F frame"))
    print(f"clip / {family}: {len(cases)} cases, {runs} case x layout runs, {halves} in RGBA16F; largest colour error vs the reference {worst[0]:.3g} ({worst[1]})")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    assert runs >= 2 * len(cases)
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"


@pytest.mark.parametrize("family", ["table", "lit", "mip", "iso lit"])
def test_unit_box_is_no_box(V, O, family):  # noqa: F811
    """lo = (0, 0, 0), hi = (1, 1, 1): bit for bit the frame and the steps of no box, in all four families, on every layout and policy."""
    cams = [O.camera_blob(*CC.CAMERAS[k]) for k in ("orbit", "eye in box", "axis")]
    for volume in ("standin32", "fog f16"):
        for lay in _layouts(O, volume):
            ctx = _context(V, O, family, volume, lay, None)
            try:
                for cam in cams:
                    for _, fl in _policies(V)[:3]:
                        ctx.set_clip_box(None)
                        assert ctx.clip_box is None
                        a = _render(V, ctx, cam, 0.5, fl | V.RENDER_COUNT)
                        ctx.set_clip_box(*CC.UNIT)
                        assert ctx.clip_box == CC.UNIT
                        b = _render(V, ctx, cam, 0.5, fl | V.RENDER_COUNT)
                        assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1] == b[1]).all(), (family, volume, lay)
                        assert a[1].max() > 0
            finally:
                ctx.close()


def test_state_round_trip_refusals_and_the_built_in_family(V, O):  # noqa: F811
    vol = CC.volumes(O)["standin32"]
    cam = O.camera_blob(*CC.CAMERAS["orbit"])
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        # before a volume: it is host state
        assert ctx.clip_box is None
        ctx.set_clip_box(*CC.ROI)
        lo, hi = ctx.clip_box
        assert lo == tuple(float(np.float32(v)) for v in CC.ROI[0]) and hi == tuple(float(np.float32(v)) for v in CC.ROI[1])
        V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
        assert ctx.clip_box == (lo, hi)  # it stays in force across uploads
        # invalid boxes are refused by the library, and the old box is kept
        L, h = V.native.lib(), ctx.handle
        for blo, bhi in (((0.5, 0.0, 0.0), (0.5, 1.0, 1.0)), ((0.6, 0.0, 0.0), (0.5, 1.0, 1.0)), ((-0.1, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.5, 1.0)),
                         ((0.0, float("nan"), 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, float("inf")))):
            b = V.VkClipBox()
            b.lo[:], b.hi[:] = blo, bhi
            assert L.vk_set_clip_box(h, C.byref(b)) == -1 and b"vk_set_clip_box" in L.vk_last_error(h), (blo, bhi)
            with pytest.raises(ValueError):
                ctx.set_clip_box(blo, bhi)
            assert ctx.clip_box == (lo, hi)
        on = C.c_int(-1)
        assert L.vk_get_clip_box(h, None, C.byref(on)) == 0 and on.value == 1 and L.vk_get_clip_box(h, None, None) == 0
        # the built-in family has no clip kernels: refused with "clip" in the message, whatever the layout; the other modes ignore the box
        ef = _empty_fraction(ctx)
        ctx.set_clip_box(None)
        assert _empty_fraction(ctx) == ef
        plain = _render(V, ctx, cam, 0.5, V.RENDER_COUNT)
        ctx.set_clip_box(*CC.ROI)
        assert _empty_fraction(ctx) == ef
        for lay in ("PACKED", "LINEAR", "BRICKED", "STAGED"):
            V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + lay))
            ctx.set_camera_blob(cam)
            with pytest.raises(V.VokselisError, match="clip") as e:
                V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5).record(ctx)
            assert e.value.code == -5  # VK_ERR_UNSUPPORTED
        V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
        ctx.set_clip_box(None)
        again = _render(V, ctx, cam, 0.5, V.RENDER_COUNT)
        assert (again[0].view(np.uint32) == plain[0].view(np.uint32)).all() and (again[1] == plain[1]).all() and plain[1].max() > 0
        # the skip maps do not depend on the box: under a table the empty fraction is the table's, box or not
        ctx.set_transfer_function(CC.table())
        ef = _empty_fraction(ctx)
        ctx.set_clip_box(*CC.HALF)
        assert _empty_fraction(ctx) == ef and 0.0 < ef < 1.0
        # a box set between frame_begin and frame_end applies to the renders recorded after it only
        clipped = _render(V, ctx, cam, 0.5, 0)[0]
        ctx.set_clip_box(None)
        unclipped = _render(V, ctx, cam, 0.5, 0)[0]
        assert (clipped.view(np.uint32) != unclipped.view(np.uint32)).any()
        left, right = (0, 0, W // 2, H), (W // 2, 0, W - W // 2, H)
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
        fid = ctx.frame_begin()
        pipe.record(ctx, left)
        ctx.set_clip_box(*CC.HALF)
        pipe.record(ctx, right)
        ctx.frame_end()
        got = ctx.read_frame(fid)
        assert (got[:, :W // 2].view(np.uint32) == unclipped[:, :W // 2].view(np.uint32)).all()
        assert (got[:, W // 2:].view(np.uint32) == clipped[:, W // 2:].view(np.uint32)).all()
        assert (clipped[:, :W // 2].view(np.uint32) != unclipped[:, :W // 2].view(np.uint32)).any()
    finally:
        ctx.close()


def test_modes_that_ignore_the_clip_box(V):  # noqa: F811
    Wm, Hm = 128, 72
    cam = _cam(V, Wm, Hm)
    xor, proc = [], []
    for box in (None, CC.ROI):
        ctx = V.Context(Wm, Hm, backbuffer=(Wm, Hm), out_format=V.OUT_RGBA32F)
        try:
            if box is not None:
                ctx.set_clip_box(*box)
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
def test_every_submission_path_gives_the_vk_render_frame_under_a_box(V, O, fmt):  # noqa: F811
    import torch

    Wb, Hb, ts = 200, 136, 32
    out = V.OUT_RGBA32F if fmt == "f32" else V.OUT_RGBA16F
    tdt = torch.float32 if fmt == "f32" else torch.float16
    cams = [_cam(V, Wb, Hb, k) for k in range(5)]
    ctx = _context(V, O, "lit", "standin32", "PACKED_PAIRS", CC.ROI, out=out, size=(Wb, Hb))
    try:
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
        singles = []
        for c in cams:
            ctx.set_camera_blob(c)
            pipe.record(ctx)
            singles.append(ctx.read_backbuffer().copy())
        assert len({s.tobytes() for s in singles}) == len(cams) and all(s[..., :3].max() > 0 for s in singles)
        ctx.set_clip_box(None)
        ctx.set_camera_blob(cams[2])
        pipe.record(ctx)
        assert (ctx.read_backbuffer().view(np.uint8) != singles[2].view(np.uint8)).any()
        # the active tiles: fewer under the region of interest than without it
        n_plain = ctx.partition_active(ts)[0]
        ctx.set_clip_box(*CC.ROI)
        n_roi = ctx.partition_active(ts)[0]
        assert 0 < n_roi < n_plain, (n_roi, n_plain)
        # tiles: the frame in four vk_render calls
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        for tile in ((0, 0, 128, 64), (128, 0, 72, 64), (0, 64, 128, 72), (128, 64, 72, 72)):
            pipe.record(ctx, tile)
        assert (ctx.read_backbuffer().view(np.uint8) == singles[2].view(np.uint8)).all()
        # whole-frame batch
        B = len(cams)
        frames = _synced(torch.zeros((B, Hb, Wb, 4), dtype=tdt, device="cuda"))
        V.render_batch(ctx, pipe, cams, frames.data_ptr(), tile_size=ts)
        ctx.sync()
        got = frames.cpu().numpy()
        for k in range(B):
            assert (got[k].view(np.uint8) == singles[k].view(np.uint8)).all(), ("batch", k)
        # compact batches + vk_untile_batch for N ranks emulated on this GPU
        for nr in (2, 3):
            cap = V.partition_slots(Wb, Hb, ts, nr, 0)
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
        # vk_render_partition at 2 and 3 ranks on this GPU, gathered and un-tiled
        ctx.set_camera_blob(cams[4])
        for nr in (2, 3):
            slots = V.partition_slots(Wb, Hb, ts, nr)
            part = _synced(torch.full((nr, slots, ts, ts, 4), float("nan"), dtype=tdt, device="cuda"))
            for r in range(nr):
                pipe.record_partition(ctx, ts, r, nr, part[r].data_ptr())
            V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
            V.native.check(ctx.handle, V.native.lib().vk_untile(ctx.handle, part.data_ptr(), ts, nr, slots))
            assert (ctx.read_backbuffer().view(np.uint8) == singles[4].view(np.uint8)).all(), ("partition", nr)
        # fused present == render + vk_present under the rule of test_frames_gpu.py
        ctx.set_camera_blob(cams[1])
        pipe.record(ctx)
        ctx.render()
        bb0, two_pass = ctx.read_backbuffer().copy(), _shot(ctx)
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5, flags=V.RENDER_PRESENT).record(ctx)
        bb1, fused = ctx.read_backbuffer(), _shot(ctx)
        assert (bb1.view(np.uint8) == bb0.view(np.uint8)).all() and (bb0.view(np.uint8) == singles[1].view(np.uint8)).all()
        centre = _centred(Hb)[:, None] & _centred(Wb)[None, :]
        d = np.abs(fused.astype(np.int32) - two_pass.astype(np.int32)).max(axis=2)
        assert (d[centre[:d.shape[0], :d.shape[1]]] == 0).all() and d.max() <= 1
        assert fused[..., :3].max() > 30
    finally:
        ctx.close()
    # frames in flight at K = 3; the box goes off between frames without a drain: each frame is the single render under its own box
    ctx = _context(V, O, "lit", "standin32", "PACKED_PAIRS", CC.ROI, out=out, size=(Wb, Hb))
    try:
        ctx.frames_in_flight(3)
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
        ctx.set_clip_box(None)
        ctx.set_camera_blob(cams[4])
        fid = ctx.frame_begin()
        pipe.record(ctx)
        ctx.frame_end()
        assert not (ctx.read_frame(fid).view(np.uint8) == singles[4].view(np.uint8)).all()
    finally:
        ctx.close()


def test_group_render_under_fake_rccl_follows_the_clip_box(V):  # noqa: F811
    import __graft_entry__ as g

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VK_RCCL_LIB=g.build_fake_rccl())
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "clip_shim_group_check.py")], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "clip_shim_group_check: OK" in r.stdout and r.stdout.count("under a clip box") == 2, r.stdout


def test_cpp_host_bonsai_clip(V, tmp_path):  # noqa: F811
    """bonsai --clip X0 Y0 Z0 X1 Y1 Z1 writes the PPM the Python host presents under the same state; --clip alone is refused."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(g.ROOT, "vokselis_amd", "_lib", "bonsai")
    Wc, Hc = 320, 180
    ppm = tmp_path / "bonsai.ppm"
    r = subprocess.run([exe, "--frames", "1", "--size", f"{Wc}x{Hc}", "--dt", "1.0", "--iso", "0.25", "--headlight", "--clip", "0.5", "0", "0", "1", "1", "1", "--ppm", str(ppm)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    hdr, data = ppm.read_bytes().split(b"\n255\n", 1)
    assert hdr == f"P6\n{Wc} {Hc}".encode()
    got = np.frombuffer(data, np.uint8).reshape(Hc, Wc, 3)
    shots = []
    ctx = V.Context(Wc, Hc, V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), Wc / Hc), backbuffer=(Wc, Hc))
    try:
        ctx.set_isosurface(0.25)
        ctx.set_lighting("headlight")
        V.VolumeTexture.generate_standin(ctx)
        ctx.update()
        for box in (CC.HALF, None):
            ctx.set_clip_box(*box) if box else ctx.set_clip_box(None)
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
            ctx.render()
            shots.append(_shot(ctx)[..., :3])
    finally:
        ctx.close()
    assert (got == shots[0]).all() and shots[0].max() > 30 and (shots[0] != shots[1]).any()
    r = subprocess.run([exe, "--frames", "1", "--size", f"{Wc}x{Hc}", "--clip", "0.5", "0", "0", "1", "1", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--clip" in r.stderr
