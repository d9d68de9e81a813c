"""The present pass on the MI355X -- vk_present (present_kernel), the fused epilogue (VK_RENDER_PRESENT*: store_present) and
vk_capture_frame -- against the float64 specification (tests/np_present_reference.py) over the shared fuzz cases (tests/present_cases.py),
under the one comparison rule: a byte equals floor(q + 0.5), or either neighbour where q + 0.5 lies within DELTA of an integer.  The CPU suite
holds the case list, DELTA and the C oracle to the same reference (tests/test_present_fuzz_cpu.py).

vk_present, every case on a fresh context: the content is written into the backbuffer through the pointer vk_backbuffer_info returns (and read
back, bit for bit), vk_present(w, h, 1), both targets read through vk_present_info:
- Rgba8 against the reference under the rule; Bgra8 bytewise Rgba8 with bytes 0 and 2 exchanged; Rgba8 equal to the oracle's vo_present
  outside the undecided bytes;
- vk_capture_frame of that present: even-rounded size, 256-byte pitch, zero padding, the device target's pixels, nothing written beyond
  pitch x height; a window of width or height 1 gives an empty image and VK_OK; a destination one byte short is VK_ERR_INVALID; dst == NULL
  queries the sizes; vk_present_info before any present is VK_ERR_INVALID and every out-pointer of it is optional.
Fused: the table cases whose colours reach +-1e30 or whose volumes hold NaN / inf, and three compute-twin cases with non-finite air, rendered
with VK_RENDER_PRESENT | VK_RENDER_PRESENT_BGRA on both surface formats.  The backbuffers hold pixels no benign scene makes (asserted: NaN
pixels on both surfaces, +inf pixels on rgba16f, finite colours beyond ACESFilm's f32 overflow point on both); Rgba8 is the reference applied
to the stored backbuffer at texel centres under the rule, bytewise vk_render + vk_present on the pixels that pass samples at a centre,
Bgra8 its swap; VK_RENDER_PRESENT_ONLY leaves the backbuffer's bytes alone and presents the same image; a ring of 3 frames in flight
captured with vk_frame_capture gives it too."""
import ctypes as C
import time

import numpy as np
import pytest

import compute_cases
import np_present_reference as P
import present_cases as PC
import table_cases
from gpu_helpers import V, _DevicePtr  # noqa: F401
from test_frames_gpu import _centred

pytestmark = pytest.mark.gpu

VK_ERR_INVALID = -1


def _backbuffer_ptr(V, ctx):
    w, h, fmt, ptr = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_void_p()
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_info(ctx.handle, C.byref(w), C.byref(h), C.byref(fmt), C.byref(ptr)))
    return w.value, h.value, fmt.value, ptr.value


def _upload(V, ctx, bb):
    """Write bb's bits into the backbuffer through its device pointer (as integers: NaN payloads travel untouched)."""
    import torch

    w, h, fmt, ptr = _backbuffer_ptr(V, ctx)
    assert (w, h) == (bb.shape[1], bb.shape[0]) and fmt == (V.OUT_RGBA16F if bb.dtype == np.float16 else V.OUT_RGBA32F) and ptr
    ints = np.ascontiguousarray(bb).view(np.int16 if bb.dtype == np.float16 else np.int32)
    ctx.sync()
    dst = torch.as_tensor(_DevicePtr(ptr, ints.shape, "<i2" if bb.dtype == np.float16 else "<i4"), device="cuda")
    dst.copy_(torch.from_numpy(ints))
    torch.cuda.synchronize()  # (torch's stream and the context's do not order each other)
    back = ctx.read_backbuffer()
    assert back.dtype == bb.dtype and (back.view(ints.dtype) == ints).all(), "the backbuffer does not hold what was written through its pointer"


def _present(V, ctx, w, h):
    V.native.check(ctx.handle, V.native.lib().vk_present(ctx.handle, w, h, 1))
    rgba, bgra = ctx.present_targets()
    assert rgba.shape == (h, w, 4) and bgra is not None and bgra.shape == (h, w, 4)
    return rgba, bgra


def _check_capture(V, ctx, rgba, fails, what):
    """vk_capture_frame of the current present against the device target `rgba`."""
    lib, (h, w) = V.native.lib(), rgba.shape[:2]
    cw, ch, pitch = C.c_uint32(7), C.c_uint32(7), C.c_uint32(7)
    V.native.check(ctx.handle, lib.vk_capture_frame(ctx.handle, None, 0, C.byref(cw), C.byref(ch), C.byref(pitch)))  # dst == NULL: a query
    unpadded = 4 * (w - w % 2)
    if (cw.value, ch.value, pitch.value) != (w - w % 2, h - h % 2, unpadded + (256 - unpadded % 256) % 256):
        fails.append((what, f"capture sizes {(cw.value, ch.value, pitch.value)}"))
        return
    n = pitch.value * ch.value
    buf = np.full(n + 64, 0xAB, np.uint8)
    rc = lib.vk_capture_frame(ctx.handle, buf.ctypes.data, n, None, None, None)
    if rc != V.native.VK_OK:
        fails.append((what, f"capture returned {rc}"))
        return
    if not (buf[n:] == 0xAB).all():
        fails.append((what, "capture wrote beyond pitch x height"))
    if n:
        rows = buf[:n].reshape(ch.value, pitch.value)
        if not (rows[:, :unpadded].reshape(ch.value, cw.value, 4) == rgba[:ch.value, :cw.value]).all():
            fails.append((what, "captured pixels differ from the device target"))
        if not (rows[:, unpadded:] == 0).all():
            fails.append((what, "capture padding is not zero"))
        if lib.vk_capture_frame(ctx.handle, buf.ctypes.data, n - 1, None, None, None) != VK_ERR_INVALID:
            fails.append((what, "a destination one byte short was accepted"))
    elif min(w, h) != 1:
        fails.append((what, "empty capture of a window wider and taller than 1"))


def _report(name, fails):
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    print(f"{name}: {len(fails)} mismatches")
    assert not fails, f"{name}: {len(fails)} mismatches; first: {fails[0]}"


def _judge(got, q, fails, what, label):
    wrong, und = P.judge(got, q, PC.DELTA)
    if wrong.any():
        y, x, ch = (int(v[0]) for v in np.nonzero(wrong))
        fails.append((what, f"{label}: {int(wrong.sum())} wrong bytes; first at ({x}, {y}) channel {ch}: byte {got[y, x, ch]}, q = {q[y, x, ch]!r}"))
    d = np.abs(got.astype(np.float64) - q)[~und]
    return und, (float(d.max()) if d.size else 0.0)


def test_present_info_before_any_present(V):
    lib = V.native.lib()
    ctx = V.Context(8, 8, backbuffer=(8, 8), out_format=V.OUT_RGBA32F)
    try:
        w = C.c_uint32()
        assert lib.vk_present_info(ctx.handle, C.byref(w), None, None, None) == VK_ERR_INVALID
        with pytest.raises(V.VokselisError):
            ctx.present_targets()
        V.native.check(ctx.handle, lib.vk_present(ctx.handle, 6, 4, 0))
        V.native.check(ctx.handle, lib.vk_present_info(ctx.handle, None, None, None, None))  # every out-pointer is optional
        rgba, bgra = ctx.present_targets()
        assert rgba.shape == (4, 6, 4) and bgra is None  # no present has asked for the surface copy
        V.native.check(ctx.handle, lib.vk_present(ctx.handle, 6, 4, 1))
        rgba, bgra = ctx.present_targets()
        assert bgra is not None and (bgra == P.bgra_of(rgba)).all()
    finally:
        ctx.close()


def test_present_fuzz_against_the_reference(V, O):
    start = time.perf_counter()
    fails, worst, presents, n_bytes, n_und = [], (0.0, None), 0, 0, 0
    for c in PC.cases():
        q = P.present_q(c.bb, c.w, c.h)
        with np.errstate(invalid="ignore"):
            want_oracle = O.present(c.bb.astype(np.float32), c.w, c.h)
        ctx = V.Context(c.w, c.h, backbuffer=(c.bw, c.bh), out_format=V.OUT_RGBA16F if c.half else V.OUT_RGBA32F)
        try:
            _upload(V, ctx, c.bb)
            rgba, bgra = _present(V, ctx, c.w, c.h)
            presents += 1
            und, err = _judge(rgba, q, fails, c, "Rgba8 against the reference")
            if err > worst[0]:
                worst = (err, c)
            n_bytes += rgba.size
            n_und += int(und.sum())
            if not (bgra == P.bgra_of(rgba)).all():
                fails.append((c, f"Bgra8 is not Rgba8 with bytes 0 and 2 exchanged at {int((bgra != P.bgra_of(rgba)).any(axis=2).sum())} pixels"))
            if not (rgba == want_oracle)[~und].all():
                fails.append((c, f"Rgba8 differs from the oracle's vo_present at {int(((rgba != want_oracle) & ~und).sum())} decided bytes"))
            _check_capture(V, ctx, rgba, fails, c)
        finally:
            ctx.close()
    elapsed = time.perf_counter() - start
    print(f"\npresent fuzz: {len(PC.cases())} cases, {presents} presents, {n_bytes} bytes ({n_und} undecided), {elapsed:.1f} s; largest |byte - q| "
          f"outside the undecided band {worst[0]:.6f} ({worst[1]})")
    _report("vk_present", fails)
    assert presents == PC.N_CASES and worst[0] <= 0.5 + PC.DELTA


# ---- the fused epilogue on backbuffers the marches make of edge data ----------------------------------------------------------------------

def _fused_cases(V, O):
    """(name, W, H, make context(out_format), mode, camera blob, dt, must not be benign).  The table cases are candidates: colours at +-1e30
    or a volume that holds NaN / inf somewhere may still render a benign frame (a domain under which every cell is clear, rays that miss
    those voxels); they run all the same, and at least half of the runs must hold a backbuffer no benign scene makes.  The compute-twin cases
    are built to make NaN and must."""
    from test_compute_fuzz_gpu import _context as compute_context
    from test_table_fuzz_gpu import _context as table_context

    out = []
    for c in table_cases.cases(O):
        nonfinite = c.f16 and not np.isfinite(c.vol.astype(np.float32)).all()
        if c.tile is None and (c.big or nonfinite):
            out.append(("table " + c.name, c.W, c.H, (lambda fmt, c=c: table_context(V, c, "PACKED", fmt)), V.MODE_NAIVE_TRILINEAR,
                        O.camera_blob(*c.cam), c.dt, False))
    twin = [c for c in compute_cases.cases(O) if "non-finite air" in c.tags and c.tile is None][:3]
    assert len(twin) == 3
    for c in twin:
        out.append(("compute " + c.name, c.W, c.H, (lambda fmt, c=c: compute_context(V, c, "LINEAR", fmt)), V.MODE_COMPUTE_NEAREST,
                    O.camera_blob(*c.cam), c.dt, True))
    return out


def _same_bits(a, b):
    with np.errstate(invalid="ignore"):
        return (a.view(np.uint8) == b.view(np.uint8)).all() or bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def test_fused_present_on_edge_backbuffers(V, O):
    start = time.perf_counter()
    lib = V.native.lib()
    fails, worst, renders, n_inf, n_nan, n_big, benign = [], (0.0, None), 0, {}, {}, {}, 0
    cases = _fused_cases(V, O)
    assert len(cases) >= 8, len(cases)
    for name, W, H, make, mode, cam, dt, by_output in cases:
        for fmt in (V.OUT_RGBA16F, V.OUT_RGBA32F):
            what = (name, "rgba16f" if fmt == V.OUT_RGBA16F else "rgba32f")
            ctx = make(fmt)
            try:
                ctx.set_camera_blob(cam)

                def draw(flags):
                    V.RaycastPipeline(mode, dt_scale=dt, flags=flags).record(ctx)

                draw(0)
                bb0 = ctx.read_backbuffer().copy()
                two_pass, _ = _present(V, ctx, W, H)
                V.native.check(ctx.handle, lib.vk_backbuffer_clear(ctx.handle))
                draw(V.RENDER_PRESENT | V.RENDER_PRESENT_BGRA)
                bb1 = ctx.read_backbuffer().copy()
                fused, bgra = ctx.present_targets()
                renders += 2
                with np.errstate(invalid="ignore"):
                    v = bb0.astype(np.float64)
                n_inf[fmt] = n_inf.get(fmt, 0) + int(np.isposinf(v[..., :3]).any(axis=2).sum())
                n_nan[fmt] = n_nan.get(fmt, 0) + int(np.isnan(v[..., :3]).any(axis=2).sum())
                n_big[fmt] = n_big.get(fmt, 0) + int((np.abs(v[..., :3]) >= float(PC.overflow_points()[1])).any(axis=2).sum())
                if np.isfinite(v).all() and np.abs(v).max() <= 1.0:
                    benign += 1
                    if by_output:
                        fails.append((what, "a benign backbuffer (all finite, within [0, 1]): the case proves nothing"))
                if not _same_bits(bb1, bb0):
                    fails.append((what, "VK_RENDER_PRESENT changed the backbuffer"))
                q = np.empty(v.shape)  # the reference at texel centres: the stored value itself
                q[..., :3], q[..., 3] = P.tone_q(v[..., :3]), P.tone_q(v[..., 3], alpha=True)
                _, err = _judge(fused, q, fails, what, "fused Rgba8 against the reference")
                if err > worst[0]:
                    worst = (err, what)
                centre = _centred(H)[:, None] & _centred(W)[None, :]
                if not (fused[centre] == two_pass[centre]).all():
                    n_diff = int((fused != two_pass).any(axis=2)[centre].sum())
                    fails.append((what, f"fused differs from vk_render + vk_present at {n_diff} centred pixels"))
                if not (bgra == P.bgra_of(fused)).all():
                    fails.append((what, "fused Bgra8 is not the swap of Rgba8"))
                _check_capture(V, ctx, fused, fails, what)
                # PRESENT_ONLY: the backbuffer keeps the bytes it held, the image is the same
                V.native.check(ctx.handle, lib.vk_backbuffer_clear(ctx.handle))
                cleared = ctx.read_backbuffer().copy()
                draw(V.RENDER_PRESENT_ONLY)
                renders += 1
                if not (ctx.read_backbuffer().view(np.uint8) == cleared.view(np.uint8)).all():
                    fails.append((what, "VK_RENDER_PRESENT_ONLY wrote the backbuffer"))
                if not (ctx.present_targets()[0] == fused).all():
                    fails.append((what, "VK_RENDER_PRESENT_ONLY presents another image"))
            finally:
                ctx.close()
            # a ring of three frames in flight: every frame still held presents that image
            ctx = make(fmt)
            try:
                ctx.frames_in_flight(3)
                ids = []
                for _ in range(4):
                    ctx.set_camera_blob(cam)
                    ids.append(ctx.frame_begin())
                    V.RaycastPipeline(mode, dt_scale=dt, flags=V.RENDER_PRESENT | V.RENDER_PRESENT_BGRA).record(ctx)
                    ctx.frame_end()
                    renders += 1
                for fid in ids[1:]:
                    buf, dims = ctx.capture_frame_of(fid)
                    rows = np.frombuffer(buf, np.uint8).reshape(dims.height, dims.padded_bytes_per_row)
                    shot = rows[:, :dims.unpadded_bytes_per_row].reshape(dims.height, dims.width, 4)
                    if not (shot == fused[:dims.height, :dims.width]).all():
                        fails.append((what, f"frame {fid} of the ring presents another image"))
            finally:
                ctx.close()
    elapsed = time.perf_counter() - start
    print(f"\nfused present fuzz: {len(cases)} cases x 2 formats, {renders} renders, {elapsed:.1f} s; +inf pixels {n_inf}, NaN pixels {n_nan}, "
          f"values beyond the overflow point {n_big}, benign backbuffers {benign}; largest |byte - q| outside the undecided band "
          f"{worst[0]:.6f} ({worst[1]})")
    # NaN pixels on both surfaces; +inf pixels on rgba16f (where every colour above 65504 is stored as +inf: a table colour of 1e30 is ~3e12
    # after the march's sRGB step); on both surfaces colours beyond the point where ACESFilm's quadratics overflow (a table colour of -1e30
    # leaves the march's sRGB step, on its linear branch, as ~-1e31: finite on rgba32f, -inf on rgba16f)
    assert n_nan.get(V.OUT_RGBA16F, 0) > 0 and n_nan.get(V.OUT_RGBA32F, 0) > 0 and n_inf.get(V.OUT_RGBA16F, 0) > 0, (n_inf, n_nan)
    assert n_big.get(V.OUT_RGBA16F, 0) > 0 and n_big.get(V.OUT_RGBA32F, 0) > 0, n_big
    assert benign <= len(cases), (benign, 2 * len(cases))
    _report("fused present", fails)
    assert worst[0] <= 0.5 + PC.DELTA
