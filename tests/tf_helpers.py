"""Shared by the transfer-function tests (test_transfer_cpu.py, test_transfer_gpu.py): the C restatement of the march under a table
(tests/tf_restatement.c, linked against the oracle), the host's table constants, and the tables the tests use."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_restatement(out_dir, O):
    """Compile tests/tf_restatement.c against the oracle's library (built by the O fixture); returns the loaded CDLL."""
    so_oracle = O.build()
    so = os.path.join(str(out_dir), "libtf_restatement.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-o", so,
                    os.path.join(ROOT, "tests", "tf_restatement.c"), so_oracle, "-Wl,-rpath," + os.path.dirname(so_oracle), "-lm"], check=True)
    L = C.CDLL(so)
    L.tfr_render.restype = C.c_int
    return L


def tf_constants(n, lo, hi, r8):
    """vk_tf.hpp: tf_constants -- k1, k2 in double, each rounded once to f32."""
    span, nm1 = float(hi) - float(lo), float(n) - 1.0
    return float(np.float32(nm1 / (span * (255.0 if r8 else 1.0)))), float(np.float32(-float(lo) * nm1 / span))


def restate(L, O, cam_blob, vol, W, H, *, dt=1.0, table=None, domain=(0.0, 1.0), tile=None):
    """Frame (rgba f32 [H, W, 4], steps u32 [H, W]) of the restatement; pixels outside `tile` stay 0."""
    cu = O.camera_from_blob(cam_blob)
    v = np.ascontiguousarray(vol)
    r8 = v.dtype == np.uint8
    if not r8:
        v = v.view(np.uint16)
    nz, ny, nx = v.shape
    out = np.zeros((H, W, 4), np.float32)
    steps = np.zeros((H, W), np.uint32)
    tx, ty, tw, th = (0, 0, W, H) if tile is None else tile
    if table is None:
        tp, n, k1, k2 = None, 0, 0.0, 0.0
    else:
        t = np.ascontiguousarray(table, np.float32)
        n = t.shape[0]
        lo, hi = np.float32(domain[0]), np.float32(domain[1])
        k1, k2 = tf_constants(n, lo, hi, r8)
        tp = t.ctypes.data_as(C.POINTER(C.c_float))
    rc = L.tfr_render(C.byref(cu), C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(0 if r8 else 1),
                      C.c_uint32(W), C.c_uint32(H), C.c_uint32(tx), C.c_uint32(ty), C.c_uint32(tw), C.c_uint32(th), C.c_float(dt), tp,
                      C.c_uint32(n), C.c_float(k1), C.c_float(k2), C.c_void_p(out.ctypes.data), C.c_void_p(steps.ctypes.data))
    assert rc == 0
    return out, steps


def zero_band_table(n=256):
    """Alpha exactly 0 below 0.1 (the built-in transfer's zero band), then a ramp through a blue-to-orange palette."""
    x = np.arange(n) / (n - 1)
    a = np.clip((x - 0.1) / 0.9, 0.0, 1.0) ** 2 * 0.8
    a[x < 0.1] = 0.0
    rgb = np.stack([0.2 + 0.8 * x, 0.3 + 0.4 * np.sin(3.0 * x) ** 2, 1.0 - 0.7 * x], axis=1)
    return np.concatenate([rgb, a[:, None]], axis=1).astype(np.float32)


def band_pass_table(n=256, lo=0.45, hi=0.6):
    """Opaque only in a narrow band of values (the trunk of the bonsai stand-in): most cells become empty."""
    x = np.arange(n) / (n - 1)
    a = np.where((x >= lo) & (x <= hi), 0.6, 0.0)
    rgb = np.stack([np.full(n, 0.9), 0.5 + 0.5 * x, np.full(n, 0.1)], axis=1)
    return np.concatenate([rgb, a[:, None]], axis=1).astype(np.float32)


def single_entry_table(n=256, j=40):
    t = np.zeros((n, 4), np.float32)
    t[:, 0:3] = 0.5
    t[j, 3] = 0.7
    return t
