"""Shared by the resample tests: the C restatement (tests/resample_restatement.c, built with -ffp-contract=off), a case through it, the
bitwise comparison of two dense volumes, the layouts of each format with their upload, and a case as the library's request."""
import ctypes as C
import os
import subprocess

import numpy as np

import resample_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = {"nearest": 0, "linear": 1, "area": 2}
LAYOUTS = {"u8": ("LINEAR", "PACKED", "PACKED_PAIRS"), "f16": ("LINEAR", "PACKED"), "u16": ("LINEAR", "PACKED")}


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libresample_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "resample_restatement.c"), "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.resample_restate.restype = C.c_int
    return L


def restate(L, vol, kind, box, mode, dims, out_kind, window):
    """The restatement's dense output [nz, ny, nx] in the output's dtype, or None where the rule refuses."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    b, d = np.array(box, np.uint32), np.array(dims, np.uint32)
    out = np.zeros((dims[2], dims[1], dims[0]), RC.DTYPE[out_kind])
    lo, hi = (0.0, 1.0) if window is None else window
    rc = L.resample_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(RC.FMT[kind]), C.c_void_p(b.ctypes.data), C.c_int(MODE[mode]),
                            C.c_void_p(d.ctypes.data), C.c_int(RC.FMT[out_kind]), C.c_int(0 if window is None else 1), C.c_float(lo), C.c_float(hi), C.c_void_p(out.ctypes.data))
    return out if rc == 0 else None


def restate_case(L, c):
    return restate(L, c.vol, c.kind, c.box, c.mode, c.dims, c.out, c.window)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def differences(got, ref):
    """A short description of where two dense volumes differ (empty: bitwise equal)."""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return f"shape / dtype {got.shape} {got.dtype} != {ref.shape} {ref.dtype}"
    bad = np.argwhere(raw(got) != raw(ref))
    if len(bad) == 0:
        return ""
    z, y, x = bad[0]
    return f"{len(bad)} of {got.size} voxels differ, first at (x, y, z) = ({x}, {y}, {z}): {raw(got)[z, y, x]:#x} != {raw(ref)[z, y, x]:#x}"


def upload(V, ctx, vol, kind, layout):
    kw = dict(fmt=V.FMT_R16_UNORM) if kind == "u16" else {}
    return V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout), **kw)


def request(V, c, install=False, out=True, layout=None):
    """A case as the library's request, and its box (None under the clip box or for the whole volume)."""
    from vokselis_amd.resample import resample_request

    d = (c.vol.shape[2], c.vol.shape[1], c.vol.shape[0])
    box = "clip" if c.clip is not None else (None if c.box == (0, 0, 0) + d else (c.box[:3], c.box[3:]))
    req = resample_request(c.dims, c.mode, None if c.out == c.kind else c.out, c.window, layout, box, install, out)
    vb = None if box in (None, "clip") else V.VkVoxelBox(*c.box)
    return req, vb


def resample_dense(V, ctx, req, vb, dims, out_kind):
    """vk_volume_resample with dense_out; returns (rc, out, VkResampleResult)."""
    from vokselis_amd import _native as N

    out = np.zeros((dims[2], dims[1], dims[0]), RC.DTYPE[out_kind])
    res = N.VkResampleResult()
    rc = N.lib().vk_volume_resample(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, C.c_void_p(out.ctypes.data), C.byref(res))
    return rc, out, res
