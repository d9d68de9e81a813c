"""Shared by the isosurface tests: the C restatement of the first-hit isosurface march (tests/iso_restatement.c, linked against the
oracle), the threshold on the kernel's scale, and the frame of a fuzz case (tests/iso_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from lit_helpers import light_vector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX, HIT, FIRST, NAN_SEEN, PINF_HIT, EQUAL = 1, 2, 4, 8, 16, 32  # iso_restatement.c's per-pixel flags


def build_restatement(out_dir, O):
    """Compile tests/iso_restatement.c against the oracle's library (built by the O fixture); returns the loaded CDLL."""
    so_oracle = O.build()
    so = os.path.join(str(out_dir), "libiso_restatement.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-o", so,
                    os.path.join(ROOT, "tests", "iso_restatement.c"), so_oracle, "-Wl,-rpath," + os.path.dirname(so_oracle), "-lm"], check=True)
    L = C.CDLL(so)
    L.isor_render.restype = C.c_int
    return L


def iso_k(iso, r8):
    """The threshold on the kernel's scale, rounded once to f32: iso * 255.0f for R8 volumes, iso for R16F."""
    with np.errstate(over="ignore"):  # (a finite iso may overflow to +-inf: the kernels' threshold does too)
        return np.float32(iso) * np.float32(255.0) if r8 else np.float32(iso)


def light_of(light):
    """The restatement's 8 floats of a case's light (keyword arguments of Context.set_lighting), or None."""
    return None if light is None else light_vector(**light)


def restate(L, O, cam_blob, vol, W, H, *, iso, colour=(1.0, 1.0, 1.0), refine=4, dt=1.0, light=None, tile=None):
    """Frame of the restatement: (rgba f32 [H, W, 4], steps u32 [H, W], a f32 [H, W], flags u32 [H, W]); pixels outside `tile` stay 0."""
    cu = O.camera_from_blob(cam_blob)
    v = np.ascontiguousarray(vol)
    r8 = v.dtype == np.uint8
    if not r8:
        v = v.view(np.uint16)
    nz, ny, nx = v.shape
    out = np.zeros((H, W, 4), np.float32)
    steps = np.zeros((H, W), np.uint32)
    a = np.zeros((H, W), np.float32)
    flags = np.zeros((H, W), np.uint32)
    tx, ty, tw, th = (0, 0, W, H) if tile is None else tile
    tw, th, tx, ty = max(0, tw + min(tx, 0)), max(0, th + min(ty, 0)), max(tx, 0), max(ty, 0)  # (a tile may start off screen)
    rgb = np.ascontiguousarray(colour, np.float32)
    lp = light_of(light)
    rc = L.isor_render(C.byref(cu), C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(0 if r8 else 1),
                       C.c_uint32(W), C.c_uint32(H), C.c_uint32(tx), C.c_uint32(ty), C.c_uint32(tw), C.c_uint32(th), C.c_float(dt),
                       C.c_float(iso_k(iso, r8)), rgb.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(refine),
                       None if lp is None else lp.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(out.ctypes.data), C.c_void_p(steps.ctypes.data),
                       C.c_void_p(a.ctypes.data), C.c_void_p(flags.ctypes.data))
    assert rc == 0, rc
    return out, steps, a, flags


def restate_case(L, O, c, tile=False):
    """The whole frame of a case (tile=True: its tile only, as the kernels render it)."""
    return restate(L, O, O.camera_blob(*c.cam), c.vol, c.W, c.H, iso=c.iso, colour=c.colour, refine=c.refine, dt=c.dt, light=c.light,
                   tile=c.tile if tile else None)
