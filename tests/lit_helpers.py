"""Shared by the lighting tests (test_lighting_cpu.py, test_lighting_gpu.py): the C restatement of the lit table march
(tests/lit_restatement.c, linked against the oracle), the host's light normalisation, and the volumes the tests use."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from tf_helpers import tf_constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_restatement(out_dir, O):
    """Compile tests/lit_restatement.c against the oracle's library (built by the O fixture); returns the loaded CDLL."""
    so_oracle = O.build()
    so = os.path.join(str(out_dir), "liblit_restatement.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-o", so,
                    os.path.join(ROOT, "tests", "lit_restatement.c"), so_oracle, "-Wl,-rpath," + os.path.dirname(so_oracle), "-lm"], check=True)
    L = C.CDLL(so)
    L.litr_render.restype = C.c_int
    L.litr_sample.restype = C.c_int
    return L


def light_vector(direction=None, ambient=0.3, diffuse=0.7, specular=0.2, shininess=32.0):
    """The 8 floats the restatement reads, as vk_set_lighting derives them (vk_light.hpp: light_desc): the direction rounded to f32, normalised
    in double, each component rounded once; "headlight" for a light at the eye."""
    if direction == "headlight":
        d, head = (0.0, 0.0, 0.0), 1.0
    else:
        x, y, z = (float(np.float32(v)) for v in direction)
        n = math.sqrt(x * x + y * y + z * z)
        d, head = (x / n, y / n, z / n), 0.0
    return np.array([*d, head, ambient, diffuse, specular, shininess], np.float32)


def _vol_args(vol):
    v = np.ascontiguousarray(vol)
    r8 = v.dtype == np.uint8
    if not r8:
        v = v.view(np.uint16)
    nz, ny, nx = v.shape
    return v, r8, nx, ny, nz


def restate(L, O, cam_blob, vol, W, H, *, table, dt=1.0, domain=(0.0, 1.0), light=None, tile=None):
    """Frame (rgba f32 [H, W, 4], steps u32 [H, W]) of the lit restatement (light: light_vector(...), or None for the unlit table); pixels
    outside `tile` stay 0."""
    cu = O.camera_from_blob(cam_blob)
    v, r8, nx, ny, nz = _vol_args(vol)
    out = np.zeros((H, W, 4), np.float32)
    steps = np.zeros((H, W), np.uint32)
    tx, ty, tw, th = (0, 0, W, H) if tile is None else tile
    t = np.ascontiguousarray(table, np.float32)
    k1, k2 = tf_constants(t.shape[0], np.float32(domain[0]), np.float32(domain[1]), r8)
    lp = None if light is None else np.ascontiguousarray(light, np.float32)
    rc = L.litr_render(C.byref(cu), C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(0 if r8 else 1),
                       C.c_uint32(W), C.c_uint32(H), C.c_uint32(tx), C.c_uint32(ty), C.c_uint32(tw), C.c_uint32(th), C.c_float(dt),
                       t.ctypes.data_as(C.POINTER(C.c_float)), C.c_uint32(t.shape[0]), C.c_float(k1), C.c_float(k2),
                       None if lp is None else lp.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(out.ctypes.data), C.c_void_p(steps.ctypes.data))
    assert rc == 0, rc
    return out, steps


def sample(L, vol, p):
    """(value, world gradient) of the restatement at the f32 position p."""
    v, r8, nx, ny, nz = _vol_args(vol)
    pp = np.asarray(p, np.float32)
    val = C.c_float()
    g = np.zeros(3, np.float32)
    rc = L.litr_sample(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(0 if r8 else 1),
                       pp.ctypes.data_as(C.POINTER(C.c_float)), C.byref(val), g.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0, rc
    return val.value, g


def sphere_u8(nx, ny=None, nz=None, radius=0.35, shell=0.2):
    """A solid ball centred in the unit cube (radius in world units), 255 inside falling linearly to 0 over a shell `shell` thick around
    the radius: a smooth density whose gradient points inwards, for checking the axes and the world scaling of the lighting."""
    ny, nz = ny or nx, nz or nx
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    r = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    return np.clip((radius + 0.5 * shell - r) / shell * 255.0, 0.0, 255.0).round().astype(np.uint8)


def solid_table(n=256, alpha=0.6, rgb=(0.8, 0.7, 0.6), lo=0.3):
    """A constant colour, alpha 0 below `lo` (the outside of the ball) and `alpha` above."""
    x = np.arange(n) / (n - 1)
    t = np.zeros((n, 4), np.float32)
    t[:, 0:3] = rgb
    t[:, 3] = np.where(x >= lo, alpha, 0.0)
    return t
