"""Shared by the geometry-pass tests: the C restatement of the pass (tests/geom_restatement.c, linked against the oracle), the miss
record, and the records of a fuzz case (tests/geom_cases.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX, HIT, FIRST, NAN_SEEN, PINF_HIT = 1, 2, 4, 8, 16  # geom_restatement.c's per-pixel flags
FMT = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.uint16): 3}
MISS = np.array([[0.0, 0.0, 0.0, np.inf], [0.0, 0.0, 0.0, 0.0]], np.float32)  # { (0, 0, 0, +inf), (0, 0, 0, 0) }


def build_restatement(out_dir, O):
    """Compile tests/geom_restatement.c against the oracle's library (built by the O fixture); returns the loaded CDLL."""
    so_oracle = O.build()
    so = os.path.join(str(out_dir), "libgeom_restatement.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"), "-o", so,
                    os.path.join(ROOT, "tests", "geom_restatement.c"), so_oracle, "-Wl,-rpath," + os.path.dirname(so_oracle), "-lm"], check=True)
    L = C.CDLL(so)
    L.geomr_render.restype = C.c_int
    return L


def iso_k(iso, dtype):
    """The threshold on the kernel's scale, rounded once to f32: iso * 255 (R8), iso * 65535 (R16_UNORM), iso (R16F)."""
    scale = {0: 255.0, 1: None, 3: 65535.0}[FMT[np.dtype(dtype)]]
    with np.errstate(over="ignore"):
        return np.float32(iso) if scale is None else np.float32(iso) * np.float32(scale)


def miss_surface(W, H):
    """A geometry surface as its allocation leaves it: the miss record in every pixel, [H, W, 2, 4] f32."""
    return np.broadcast_to(MISS, (H, W, 2, 4)).copy()


def restate(L, O, cam_blob, vol, W, H, *, iso, refine=4, dt=1.0, box=None, tile=None):
    """The restatement's records: (rec f32 [H, W, 2, 4], steps u32, a f32, flags u32: each [H, W]); pixels outside `tile` keep the miss
    record (steps, a, flags: 0).  box: (lo3, hi3); tile: (x, y, w, h), the origin may be negative."""
    cu = O.camera_from_blob(cam_blob)
    v = np.ascontiguousarray(vol)
    fmt = FMT[v.dtype]
    if fmt == 1:
        v = v.view(np.uint16)
    nz, ny, nx = v.shape
    rec = miss_surface(W, H)
    steps, flags = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    a = np.zeros((H, W), np.float32)
    tx, ty, tw, th = (0, 0, W, H) if tile is None else tile
    bp = None if box is None else np.ascontiguousarray([*box[0], *box[1]], np.float32)
    rc = L.geomr_render(C.byref(cu), C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(fmt),
                        C.c_uint32(W), C.c_uint32(H), C.c_int32(tx), C.c_int32(ty), C.c_uint32(tw), C.c_uint32(th), C.c_float(dt),
                        C.c_float(iso_k(iso, vol.dtype)), C.c_uint32(refine), None if bp is None else bp.ctypes.data_as(C.POINTER(C.c_float)),
                        C.c_void_p(rec.ctypes.data), C.c_void_p(steps.ctypes.data), C.c_void_p(a.ctypes.data), C.c_void_p(flags.ctypes.data))
    assert rc == 0, rc
    return rec, steps, a, flags


def restate_case(L, O, c, tile=False, **over):
    """The whole frame of a case (tile=True: its tile only, as the kernels render it); `over` replaces arguments."""
    kw = dict(iso=c.iso, refine=c.refine, dt=c.dt, box=c.box, tile=c.tile if tile else None)
    kw.update(over)
    return restate(L, O, O.camera_blob(*c.cam), c.vol, c.W, c.H, **kw)


def tile_mask(c):
    m = np.ones((c.H, c.W), bool)
    if c.tile is not None:
        x, y, w, h = c.tile
        m[:] = False
        m[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = True
    return m


def same_bits(a, b):
    """Elementwise: the same f32 bit patterns.  Two NaNs count as the same: which NaN an invalid operation (inf - inf, 0 * inf on a cell
    with a non-finite tap) produces is not specified -- an x86 host gives the quiet NaN with the sign set, gfx950 the one without -- so a
    NaN component can be held to "is a NaN" only.  Every other value, infinities and signed zeros included, is compared bit for bit."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
