"""Shared by the maximum-intensity-projection tests: the C restatement of the MIP march (tests/mip_restatement.c, linked against the
oracle), the grey ramp that stands for "no table", and the frame of a fuzz case (tests/mip_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from tf_helpers import tf_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT, BROKE, MAX_AT_LAST, NAN_SEEN, PINF_SEEN = 1, 2, 4, 8, 16  # mip_restatement.c's per-pixel flags
GREY_RAMP = np.array([[0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]], np.float32)


def build_restatement(out_dir, O):
    """Compile tests/mip_restatement.c against the oracle's library (built by the O fixture); returns the loaded CDLL."""
    so_oracle = O.build()
    so = os.path.join(str(out_dir), "libmip_restatement.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-o", so,
                    os.path.join(ROOT, "tests", "mip_restatement.c"), so_oracle, "-Wl,-rpath," + os.path.dirname(so_oracle), "-lm"], check=True)
    L = C.CDLL(so)
    L.mipr_render.restype = C.c_int
    return L


def table_and_domain(table, domain):
    """The table in force and its window: the implicit grey ramp over [0, 1] when no table is set."""
    if table is None:
        return GREY_RAMP, (0.0, 1.0)
    return np.ascontiguousarray(table, np.float32), domain


def restate(L, O, cam_blob, vol, W, H, *, dt=1.0, table=None, domain=(0.0, 1.0)):
    """Whole frame of the restatement: (rgba f32 [H, W, 4], steps u32 [H, W], U f32 [H, W], flags u32 [H, W])."""
    cu = O.camera_from_blob(cam_blob)
    v = np.ascontiguousarray(vol)
    r8 = v.dtype == np.uint8
    if not r8:
        v = v.view(np.uint16)
    nz, ny, nx = v.shape
    out = np.zeros((H, W, 4), np.float32)
    steps = np.zeros((H, W), np.uint32)
    U = np.zeros((H, W), np.float32)
    flags = np.zeros((H, W), np.uint32)
    t, (lo, hi) = table_and_domain(table, domain)
    n = t.shape[0]
    k1, k2 = tf_constants(n, np.float32(lo), np.float32(hi), r8)
    rc = L.mipr_render(C.byref(cu), C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(0 if r8 else 1),
                       C.c_uint32(W), C.c_uint32(H), C.c_uint32(0), C.c_uint32(0), C.c_uint32(W), C.c_uint32(H), C.c_float(dt),
                       t.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(n), C.c_float(k1), C.c_float(k2), C.c_void_p(out.ctypes.data),
                       C.c_void_p(steps.ctypes.data), C.c_void_p(U.ctypes.data), C.c_void_p(flags.ctypes.data))
    assert rc == 0
    return out, steps, U, flags


def restate_case(L, O, c):
    return restate(L, O, O.camera_blob(*c.cam), c.vol, c.W, c.H, dt=c.dt, table=c.table, domain=c.domain)
