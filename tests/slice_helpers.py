"""Shared by the slice-pass tests: the C restatement of the pass (tests/slice_restatement.c, linked against the oracle), the constants the
host forms (k1, k2, rn), and the frames of a fuzz case (tests/slice_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

from geom_helpers import same_bits  # noqa: F401  (NaN: held to "is a NaN")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSIDE, FACE, CLAMPED, NAN_PASSED, ALL_NAN, MEAN_ROUNDED = 1, 2, 4, 8, 16, 32  # slice_restatement.c's per-pixel flags
FMT = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.uint16): 3}
SCALE = {0: 255.0, 1: 1.0, 3: 65535.0}  # the kernel's scale of a format: a filtered sample is SCALE times the normalised value
REDUCE = {"max": 0, "min": 1, "mean": 2}
GREY_RAMP = np.array([[0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]], np.float32)
CLEAR = np.array([0.0, 0.0, 0.0, 1.0], np.float32)
UNIT_BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def build_restatement(out_dir, O):
    """Compile tests/slice_restatement.c against the oracle's library (built by the O fixture), as geom_helpers.build_restatement does;
    returns the loaded CDLL."""
    so_oracle = O.build()
    so = os.path.join(str(out_dir), "libslice_restatement.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-o", so,
                    os.path.join(ROOT, "tests", "slice_restatement.c"), so_oracle, "-Wl,-rpath," + os.path.dirname(so_oracle), "-lm"], check=True)
    L = C.CDLL(so)
    L.slicer_render.restype = C.c_int
    return L


def tf_constants(n, lo, hi, fmt):
    """vk_tf.hpp: tf_constants -- k1, k2 from the f32 domain in double, each rounded once to f32."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    span, nm1 = hi - lo, float(n) - 1.0
    return np.float32(nm1 / (span * SCALE[fmt])), np.float32(-lo * nm1 / span)


def table_and_domain(table, domain):
    if table is None:
        return GREY_RAMP, (0.0, 1.0)
    return np.ascontiguousarray(table, np.float32), domain


def restate(L, vol, W, H, plane, *, samples=1, reduce="max", table=None, domain=(0.0, 1.0), box=None, tile=None):
    """The restatement's frame: (rgba f32 [H, W, 4], val f32 [H, W, 2], pos f32 [H, W, 3], flags u32 [H, W]).  Pixels outside `tile` hold the
    clear colour, the zero record, zero positions and no flags -- what a cleared backbuffer and a fresh value surface hold."""
    v = np.ascontiguousarray(vol)
    fmt = FMT[v.dtype]
    if fmt == 1:
        v = v.view(np.uint16)
    nz, ny, nx = v.shape
    rgba = np.broadcast_to(CLEAR, (H, W, 4)).copy()
    val, pos, flags = np.zeros((H, W, 2), np.float32), np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.uint32)
    tx, ty, tw, th = (0, 0, W, H) if tile is None else tile
    t, (lo, hi) = table_and_domain(table, domain)
    n = t.shape[0]
    k1, k2 = tf_constants(n, lo, hi, fmt)
    bp = np.ascontiguousarray([*(box or UNIT_BOX)[0], *(box or UNIT_BOX)[1]], np.float32)
    pl = np.ascontiguousarray(plane, np.float32)
    rn = np.float32(1.0 / float(samples))
    fp = C.POINTER(C.c_float)
    rc = L.slicer_render(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(fmt), C.c_uint32(W), C.c_uint32(H),
                         C.c_int32(tx), C.c_int32(ty), C.c_uint32(tw), C.c_uint32(th), pl.ctypes.data_as(fp), C.c_uint32(samples),
                         C.c_int(REDUCE[reduce]), C.c_float(rn), bp.ctypes.data_as(fp), t.ctypes.data_as(fp), C.c_uint32(n), C.c_float(k1),
                         C.c_float(k2), C.c_void_p(rgba.ctypes.data), C.c_void_p(val.ctypes.data), C.c_void_p(pos.ctypes.data),
                         C.c_void_p(flags.ctypes.data))
    assert rc == 0, rc
    return rgba, val, pos, flags


def restate_case(L, c, tile=False, **over):
    """The whole frame of a case (tile=True: its tile only, as the kernels render it); `over` replaces arguments."""
    kw = dict(samples=c.samples, reduce=c.reduce, table=c.table, domain=c.domain, box=c.box, tile=c.tile if tile else None)
    kw.update(over)
    return restate(L, c.vol, c.W, c.H, c.plane, **kw)


def tile_mask(c):
    m = np.ones((c.H, c.W), bool)
    if c.tile is not None:
        x, y, w, h = c.tile
        m[:] = False
        m[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = True
    return m


def rel_err(got, ref):
    """Colour error relative to max(1, |ref|), as the table kernels' bar is applied."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.abs(got - ref) / np.maximum(1.0, np.abs(ref))


def vk_slice(V, c, **over):
    """The case's plane as a VkSlice."""
    return V.Slice.raw(c.plane[0], c.plane[1], c.plane[2], c.plane[3], over.get("samples", c.samples), over.get("reduce", c.reduce))
