"""Shared by the shadow tests: the C restatement of the first-hit isosurface march with light-direction shadows
(tests/shadow_restatement.c, linked against the oracle) and the frame of a fuzz case (tests/shadow_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from lit_helpers import light_vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# shadow_restatement.c's per-pixel flags
BOX, HIT, FIRST, CAST, SHADOWED, MISS, ZERO, NAN_SEEN, PINF_HIT = 1, 2, 4, 8, 16, 32, 64, 128, 256
FMT = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.uint16): 3}


def build_restatement(out_dir, O):
    """Compile tests/shadow_restatement.c against the oracle's library (built by the O fixture); returns the loaded CDLL."""
    so_oracle = O.build()
    so = os.path.join(str(out_dir), "libshadow_restatement.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-o", so,
                    os.path.join(ROOT, "tests", "shadow_restatement.c"), so_oracle, "-Wl,-rpath," + os.path.dirname(so_oracle), "-lm"], check=True)
    L = C.CDLL(so)
    L.shr_render.restype = C.c_int
    return L


def iso_k(iso, dtype):
    """The threshold on the kernel's scale, rounded once to f32: iso * 255 (R8), iso * 65535 (R16_UNORM), iso (R16F)."""
    scale = {0: 255.0, 1: None, 3: 65535.0}[FMT[np.dtype(dtype)]]
    with np.errstate(over="ignore"):
        return np.float32(iso) if scale is None else np.float32(iso) * np.float32(scale)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def restate(L, O, cam_blob, vol, W, H, *, iso, colour=(1.0, 1.0, 1.0), refine=4, dt=1.0, light=None, shadows=None, box=None, tile=None):
    """Frame of the restatement: (rgba f32 [H, W, 4], steps u32, a f32, flags u32, shadow iterations u32, nl f32: each [H, W]); pixels
    outside `tile` stay 0.  light: the keyword arguments of Context.set_lighting; shadows: (strength, bias); box: (lo3, hi3)."""
    cu = O.camera_from_blob(cam_blob)
    v = np.ascontiguousarray(vol)
    fmt = FMT[v.dtype]
    if fmt == 1:
        v = v.view(np.uint16)
    nz, ny, nx = v.shape
    out = np.zeros((H, W, 4), np.float32)
    steps, flags, iters = (np.zeros((H, W), np.uint32) for _ in range(3))
    a, nl = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    tx, ty, tw, th = (0, 0, W, H) if tile is None else tile
    tw, th, tx, ty = max(0, tw + min(tx, 0)), max(0, th + min(ty, 0)), max(tx, 0), max(ty, 0)  # (a tile may start off screen)
    rgb = np.ascontiguousarray(colour, np.float32)
    lp = None if light is None else light_vector(**light)
    sp = None if shadows is None else np.ascontiguousarray(shadows, np.float32)
    bp = None if box is None else np.ascontiguousarray([*box[0], *box[1]], np.float32)
    rc = L.shr_render(C.byref(cu), C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(fmt),
                      C.c_uint32(W), C.c_uint32(H), C.c_uint32(tx), C.c_uint32(ty), C.c_uint32(tw), C.c_uint32(th), C.c_float(dt),
                      C.c_float(iso_k(iso, vol.dtype)), _fp(rgb), C.c_uint32(refine), _fp(lp), _fp(sp), _fp(bp), C.c_void_p(out.ctypes.data),
                      C.c_void_p(steps.ctypes.data), C.c_void_p(a.ctypes.data), C.c_void_p(flags.ctypes.data), C.c_void_p(iters.ctypes.data),
                      C.c_void_p(nl.ctypes.data))
    assert rc == 0, rc
    return out, steps, a, flags, iters, nl


def restate_case(L, O, c, **over):
    """The whole frame of a case; `over` replaces arguments (shadows=None: the frame without shadows)."""
    kw = dict(iso=c.iso, colour=c.colour, refine=c.refine, dt=c.dt, light=c.light, shadows=c.shadows, box=c.box)
    kw.update(over)
    return restate(L, O, O.camera_blob(*c.cam), c.vol, c.W, c.H, **kw)
