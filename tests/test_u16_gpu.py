"""R16_UNORM volumes on the MI355X (VK_FMT_R16_UNORM): the u16 kernels of every NAIVE_TRILINEAR family over the shared
cases (tests/u16_cases.py), against the numpy references on the u16 scale (tests/np_u16_reference.py).

For every case on LINEAR and PACKED, through the Python API:
- per-pixel step counts equal the reference's; colour within the family's existing bar (TOL_UNLIT 1e-5, TOL_LIT 1e-4, the built-in march
  gpu_helpers.TOL), relative to max(1, |ref|); colour finite, alpha 1; misses exactly (0, 0, 0, 1) with 0 steps;
- the policies of test_table_fuzz_gpu (force + probe, default, no skip, safe) and the production kernel give bitwise-equal frames;
- RGBA16F output is the round-to-nearest-even of the RGBA32F frame (the cases marked `half`);
- under RENDER_PROBE_ALWAYS on PACKED, S_sampled equals the reference's count of steps in non-empty cells in the built-in, MAX and
  isosurface families.  The table and lit families are not covered: np_table_reference returns no such count (their skip maps are held to
  the numpy census below, and their steps and frames to the reference under every policy).
Then the census after every setter, vk_volume_info, upload against upload_device, the refusals, every other submission path against
vk_render, vk_group_render under the stand-in RCCL, and the bonsai host with --raw-u16."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import np_u16_reference as NU
import table_cases as TC
import u16_cases
from gpu_helpers import TOL as TOL_BUILTIN
from gpu_helpers import V, _synced  # noqa: F401
from test_frames_gpu import _centred, _shot
from test_table_fuzz_cpu import rel_err
from test_table_fuzz_gpu import TOL_LIT, TOL_UNLIT, _policies
from test_transfer_gpu import _cam, _empty_fraction

pytestmark = pytest.mark.gpu

LAYOUTS = ("LINEAR", "PACKED")


def _tol(c):
    if c.family == "builtin":
        return TOL_BUILTIN
    return TOL_LIT if c.lit else TOL_UNLIT


def _set_family(ctx, c):
    if c.table is not None:
        ctx.set_transfer_function(c.table, c.domain)
    if c.lit:
        ctx.set_lighting(**c.light)
    if c.family in ("mip", "mipgrey"):
        ctx.set_projection("max")
    if c.family == "iso":
        ctx.set_isosurface(c.iso, c.colour, c.refine)
    if c.box is not None:
        ctx.set_clip_box(*c.box)


def _context(V, c, layout, out=None, size=None):
    size = (c.W, c.H) if size is None else size
    ctx = V.Context(*size, backbuffer=size, out_format=V.OUT_RGBA32F if out is None else out)
    try:
        _set_family(ctx, c)
        V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout), fmt=V.FMT_R16_UNORM)
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


@pytest.mark.parametrize("family", u16_cases.FAMILIES)
def test_u16_cases_against_the_references(V, O, family):  # noqa: F811
    fails, worst, runs, halves, sampled = [], (0.0, None), 0, 0, 0
    cases = [c for c in u16_cases.cases(O) if c.family == family]
    assert len(cases) >= 5
    for c in cases:
        cam = O.camera_blob(*c.cam)
        ref, ref_steps, ref_live = u16_cases.reference(O, c)
        missed = ref_steps == 0
        for lay in LAYOUTS:
            what = (c, lay)
            ctx = _context(V, c, lay)
            try:
                if c.empty is not None and lay == "PACKED" and _empty_fraction(ctx) != c.empty:
                    fails.append((what, f"empty fraction {_empty_fraction(ctx)}, want {c.empty}"))
                frames = []
                for name, fl in _policies(V):
                    img, steps = _render(V, ctx, cam, c.dt, fl | V.RENDER_COUNT)
                    frames.append((name, img, steps, ctx.step_counts()))
                prod, _ = _render(V, ctx, cam, c.dt, 0)
            finally:
                ctx.close()
            runs += 1
            _, img, steps, counts = frames[0]
            if not (steps == ref_steps).all():
                fails.append((what, f"steps differ from the reference at {int((steps != ref_steps).sum())} pixels"))
            if not np.isfinite(img[..., :3]).all():
                fails.append((what, "non-finite output"))
            if not (img[..., 3] == 1.0).all():
                fails.append((what, "alpha is not 1"))
            err = float(rel_err(img[..., :3], ref).max())
            if err > _tol(c) or np.isnan(err):
                fails.append((what, f"colour error {err:.3g} > {_tol(c)}"))
            if err >= worst[0]:
                worst = (err, f"{c.name} / {lay}")
            if not ((img[missed] == [0.0, 0.0, 0.0, 1.0]).all() and (steps[missed] == 0).all()):
                fails.append((what, "a miss is not (0, 0, 0, 1) with 0 steps"))
            if counts[0] != int(ref_steps.sum()):
                fails.append((what, f"S_ref {counts[0]}, the reference steps {int(ref_steps.sum())} times"))
            if lay == "PACKED" and ref_live is not None:
                sampled += 1
                if counts[1] != int(ref_live.sum()):
                    fails.append((what, f"S_sampled {counts[1]} under PROBE_ALWAYS, the reference's non-empty steps {int(ref_live.sum())}"))
            for name, other, osteps, _ in frames[1:]:
                if not (other.view(np.uint32) == img.view(np.uint32)).all():
                    fails.append((what, f"policy '{name}' differs from '{frames[0][0]}' at {int((other.view(np.uint32) != img.view(np.uint32)).any(axis=2).sum())} pixels"))
                if not (osteps == steps).all():
                    fails.append((what, f"policy '{name}': steps differ"))
            if not (prod.view(np.uint32) == img.view(np.uint32)).all():
                fails.append((what, "the production kernel differs from the COUNT kernel"))
            if c.half:
                ctx = _context(V, c, lay, V.OUT_RGBA16F)
                try:
                    h, _ = _render(V, ctx, cam, c.dt, 0)
                finally:
                    ctx.close()
                halves += 1
                if not (h.view(np.uint16) == prod.astype(np.float16).view(np.uint16)).all():
                    fails.append((what, "RGBA16F output is not the RNE of the RGBA32F frame"))
    print(f"\nu16 {family}: {len(cases)} cases, {runs} case x layout runs, {halves} half-float, {sampled} S_sampled checks; largest colour error "
          f"{worst[0]:.3g} ({worst[1]})")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    assert runs == 2 * len(cases) and (sampled > 0 or family in ("table", "lit"))
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"


def _case(O, name):
    return next(c for c in u16_cases.cases(O) if c.name == name)


def test_census_after_every_setter_and_volume_info(V, O):  # noqa: F811
    """vk_volume_empty_fraction is the numpy census of the predicate in force; vk_volume_info reports the format and the layout."""
    rng = np.random.default_rng(5)
    table = TC.random_table(rng, 64)
    table[:6, 3] = 0.0
    for name in ("widen table", "dims33x17x65", "dims5x4x9"):
        vol = _case(O, name).vol
        nz, ny, nx = vol.shape
        for requested, got in (("PACKED", V.LAYOUT_PACKED), ("AUTO", V.LAYOUT_PACKED), ("LINEAR", V.LAYOUT_LINEAR)):
            ctx = V.Context(32, 32, backbuffer=(32, 32))
            try:
                V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + requested), fmt=V.FMT_R16_UNORM)
                dims, fmt, lay, nbytes = (C.c_uint32 * 3)(), C.c_int(), C.c_int(), C.c_size_t()
                V.native.check(ctx.handle, V.native.lib().vk_volume_info(ctx.handle, dims, C.byref(fmt), C.byref(lay), C.byref(nbytes)))
                assert tuple(dims) == (nx, ny, nz) and fmt.value == V.FMT_R16_UNORM == 3 and lay.value == got
                if got == V.LAYOUT_LINEAR:
                    assert nbytes.value == vol.nbytes and _empty_fraction(ctx) == 0.0
                    continue
                assert nbytes.value >= 16 * 8 * vol.size // 8
                builtin = NU.empty_fraction(vol)
                assert _empty_fraction(ctx) == builtin
                ctx.set_transfer_function(table, (0.0, 1.0))
                assert _empty_fraction(ctx) == NU.empty_fraction(vol, table=table)
                ctx.set_projection("max")
                assert _empty_fraction(ctx) == NU.empty_fraction(vol, table=table, mip=True)
                ctx.set_isosurface(0.45)
                assert _empty_fraction(ctx) == NU.empty_fraction(vol, iso=0.45)
                ctx.set_isosurface(None)
                assert _empty_fraction(ctx) == NU.empty_fraction(vol, table=table, mip=True)
                ctx.set_transfer_function(None)
                assert _empty_fraction(ctx) == NU.empty_fraction(vol, mip=True)
                ctx.set_projection(None)
                assert _empty_fraction(ctx) == builtin
                # ... and a volume uploaded under a state takes that state's census
                ctx.set_isosurface(0.2)
                V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED, fmt=V.FMT_R16_UNORM)
                assert _empty_fraction(ctx) == NU.empty_fraction(vol, iso=0.2)
            finally:
                ctx.close()
    assert 0.0 < NU.empty_fraction(_case(O, "widen table").vol) < 1.0


def test_upload_device_gives_the_upload_frame(V, O):  # noqa: F811
    import torch

    c = _case(O, "widen lit")
    cam = O.camera_blob(*c.cam)
    nx, ny, nz = c.dims
    for lay in LAYOUTS:
        ctx = _context(V, c, lay)
        try:
            a = _render(V, ctx, cam, c.dt, V.RENDER_COUNT)
            dev = _synced(torch.from_numpy(c.vol.view(np.int16).copy()).cuda())
            V.native.check(ctx.handle, V.native.lib().vk_volume_upload_device(ctx.handle, dev.data_ptr(), None, nx, ny, nz, V.FMT_R16_UNORM, getattr(V, "LAYOUT_" + lay)))
            b = _render(V, ctx, cam, c.dt, V.RENDER_COUNT)
            del dev  # (the library keeps a copy of its own)
            assert (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1] == b[1]).all() and a[1].max() > 0
        finally:
            ctx.close()


def test_unsupported_combinations_leave_the_state(V, O):  # noqa: F811
    c = _case(O, "widen builtin")
    cam = O.camera_blob(*c.cam)
    nx, ny, nz = c.dims
    L = V.native.lib()
    ctx = _context(V, c, "PACKED")
    try:
        h = ctx.handle
        before = _render(V, ctx, cam, c.dt, V.RENDER_COUNT)
        ef = _empty_fraction(ctx)
        for lay in ("PACKED_PAIRS", "BRICKED", "QUADS", "STAGED"):
            assert L.vk_volume_upload(h, c.vol.ctypes.data, None, nx, ny, nz, V.FMT_R16_UNORM, getattr(V, "LAYOUT_" + lay)) == -5, lay
            assert b"R16_UNORM" in L.vk_last_error(h)
        for kind in (V.GEN_FOG, V.GEN_BONSAI_STANDIN, V.GEN_FOG_DENSE_CORE):
            assert L.vk_volume_generate(h, kind, 16, 16, 16, V.FMT_R16_UNORM, 1, 20, 12, V.LAYOUT_AUTO) == -5
        assert L.vk_volume_upload(h, c.vol.ctypes.data, None, nx, ny, nz, 4, V.LAYOUT_AUTO) == -1  # no such format
        ctx.set_camera_blob(cam)
        with pytest.raises(V.VokselisError) as e:
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=c.dt, flags=V.RENDER_FAST_WALK).record(ctx)
        assert e.value.code == -5
        with pytest.raises(V.VokselisError) as e:  # COMPUTE_NEAREST answers a u16 volume as it answers an R8 one
            V.RaycastPipeline(V.MODE_COMPUTE_NEAREST).record(ctx)
        assert e.value.code == -1
        # the volume, its maps and its census are what they were
        dims, fmt, lay_ = (C.c_uint32 * 3)(), C.c_int(), C.c_int()
        V.native.check(h, L.vk_volume_info(h, dims, C.byref(fmt), C.byref(lay_), None))
        assert tuple(dims) == (nx, ny, nz) and fmt.value == V.FMT_R16_UNORM and lay_.value == V.LAYOUT_PACKED and _empty_fraction(ctx) == ef
        after = _render(V, ctx, cam, c.dt, V.RENDER_COUNT)
        assert (after[0].view(np.uint32) == before[0].view(np.uint32)).all() and (after[1] == before[1]).all() and before[1].max() > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", ["f32", "f16"])
def test_every_submission_path_gives_the_vk_render_frame(V, O, fmt):  # noqa: F811
    import torch

    Wb, Hb, ts = 200, 136, 32
    out = V.OUT_RGBA32F if fmt == "f32" else V.OUT_RGBA16F
    tdt = torch.float32 if fmt == "f32" else torch.float16
    cams = [_cam(V, Wb, Hb, k) for k in range(5)]
    c = _case(O, "widen lit" if fmt == "f32" else "widen builtin")
    ctx = _context(V, c, "PACKED", out=out, size=(Wb, Hb))
    try:
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5)
        singles = []
        for cam in cams:
            ctx.set_camera_blob(cam)
            pipe.record(ctx)
            singles.append(ctx.read_backbuffer().copy())
        assert len({s.tobytes() for s in singles}) == len(cams) and all(s[..., :3].max() > 0 for s in singles)
        ctx.set_camera_blob(cams[2])
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
        # frames in flight at K = 3
        ctx.frames_in_flight(3)
        ids = []
        for k in range(5):
            ctx.set_camera_blob(cams[k])
            fid = ctx.frame_begin()
            pipe.record(ctx)
            ctx.frame_end()
            ids.append(fid)
        assert (ctx.read_frame(ids[-1]).view(np.uint8) == singles[4].view(np.uint8)).all()
        assert (ctx.read_frame(ids[-2]).view(np.uint8) == singles[3].view(np.uint8)).all()
    finally:
        ctx.close()


def test_group_render_under_fake_rccl_on_a_u16_volume(V):  # noqa: F811
    import __graft_entry__ as g

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VK_RCCL_LIB=g.build_fake_rccl())
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "u16_shim_group_check.py")], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "u16_shim_group_check: OK" in r.stdout and r.stdout.count("on a u16 volume") == 2, r.stdout


def test_cpp_host_bonsai_raw_u16(V, O, tmp_path):  # noqa: F811
    """bonsai --raw-u16 FILE --dims NX NY NZ writes the PPM the Python host presents of the same volume under the same state; a file of the
    wrong size is refused."""
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(g.ROOT, "vokselis_amd", "_lib", "bonsai")
    Wc, Hc, dims = 320, 180, (48, 40, 56)
    rng = np.random.default_rng(11)
    vol = np.minimum(O.volume_standin_u8(dims).astype(np.int64) * 257 + rng.integers(0, 256, dims[::-1]), 65535).astype(np.uint16)
    raw, ppm = tmp_path / "vol_u16.raw", tmp_path / "bonsai.ppm"
    vol.tofile(raw)
    args = ["--frames", "1", "--size", f"{Wc}x{Hc}", "--dt", "1.0", "--raw-u16", str(raw), "--dims", *map(str, dims)]
    state = ["--iso", "0.4", "--headlight", "--clip", "0.5", "0", "0", "1", "1", "1"]
    r = subprocess.run([exe, *args, *state, "--ppm", str(ppm)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    hdr, data = ppm.read_bytes().split(b"\n255\n", 1)
    assert hdr == f"P6\n{Wc} {Hc}".encode()
    got = np.frombuffer(data, np.uint8).reshape(Hc, Wc, 3)
    ctx = V.Context(Wc, Hc, V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), Wc / Hc), backbuffer=(Wc, Hc))
    try:
        ctx.set_isosurface(0.4)
        ctx.set_lighting("headlight")
        ctx.set_clip_box((0.5, 0.0, 0.0), (1.0, 1.0, 1.0))
        V.VolumeTexture.from_raw(ctx, str(raw), dims=dims, dtype=np.uint16)
        ctx.update()
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
        ctx.render()
        want = _shot(ctx)[..., :3]
    finally:
        ctx.close()
    assert (got == want).all() and want.max() > 30
    # the built-in transfer and the maximum projection run too; the wrong dims are refused
    for extra in ([], ["--mip"]):
        r = subprocess.run([exe, *args, *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Avg frame time" in r.stdout, r.stderr
    r = subprocess.run([exe, "--frames", "1", "--size", f"{Wc}x{Hc}", "--raw-u16", str(raw), "--dims", "48", "40", "55"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "expected" in r.stderr
