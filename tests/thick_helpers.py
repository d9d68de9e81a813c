"""Shared by the local-thickness tests: the C restatement (tests/thick_restatement.c), a case through it and through the numpy reference,
the comparison of two results, and a case as the library's request.  Layouts and uploads are the label tests' (label_helpers)."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_helpers as LH
import np_thick_reference as NT
import thick_cases as TC

ROOT = LH.ROOT


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libthick_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "thick_restatement.c"), "-lm"], check=True)
    L = C.CDLL(so)
    L.thick_restate.restype = C.c_int
    return L


def restate(L, vol, kind, lo, hi, spacing, max_radius, gain=0.0, fill_out=0.0, box=None):
    """(t2 uint32 [nz, ny, nx], dense, result uint64 [5]: n_foreground, max_t2, n_saturated, sum_t2, the bits of the gain used); None when
    the restatement refuses the volume for overflow."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    b = np.array(box if box is not None else LH.whole(v), np.uint32)
    sp = np.array(spacing, np.uint32)
    t2, dense, result = np.zeros(v.shape, np.uint32), np.zeros_like(v), np.zeros(5, np.uint64)
    rc = L.thick_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(LH.FMT[kind]), C.c_float(lo), C.c_float(hi), C.c_void_p(sp.ctypes.data),
                         C.c_float(max_radius), C.c_float(gain), C.c_float(fill_out), C.c_void_p(b.ctypes.data), C.c_void_p(t2.ctypes.data), C.c_void_p(dense.ctypes.data),
                         C.c_void_p(result.ctypes.data))
    if rc == -2:
        return None
    assert rc == 0, rc
    return t2, dense, result


def restate_case(L, c):
    return restate(L, c.vol, c.kind, c.lo, c.hi, c.spacing, c.max_radius, c.gain, c.fill_out, c.box)


def reference_case(c):
    return NT.apply(c.vol, c.kind, c.lo, c.hi, c.spacing, c.max_radius, c.gain, c.fill_out, c.box)


def differences(got, ref):
    """Where two results (t2, dense, result) differ, in words (empty: bitwise equal)."""
    if got is None or ref is None:
        return "" if got is None and ref is None else "one of the two refuses the case"
    out = []
    for name, g, r in zip(("t2", "dense", "result"), got, ref):
        if (g is None) != (r is None):
            out.append(f"{name}: present in one result only")
            continue
        if g is None:
            continue
        g, r = LH.raw(g), LH.raw(r)
        if g.shape != r.shape or g.dtype != r.dtype:
            out.append(f"{name}: shape / dtype {g.shape} {g.dtype} != {r.shape} {r.dtype}")
        elif (g != r).any():
            at = np.argwhere(g != r)[0]
            out.append(f"{name}: {int((g != r).sum())} of {g.size} differ, first at {tuple(int(v) for v in at)} (array order): {g[tuple(at)]} != {r[tuple(at)]}")
    return "; ".join(out)


def request(c, install=False):
    """A case as the library's request (with VK_THICK_CLIP_BOX where the case's box is the clip box) and its box argument."""
    from vokselis_amd import _native as N
    from vokselis_amd.thickness import thickness_request

    req = thickness_request(c.lo, c.hi, max_radius=c.max_radius, spacing=c.spacing, box="clip" if c.clip is not None else None, gain=c.gain if c.gain != 0.0 else None,
                            fill_out=c.fill_out, install=install)
    vb = N.VkVoxelBox(*c.box) if c.box is not None and c.clip is None else None
    return req, vb


def result_array(res):
    return np.array([res.n_foreground, res.max_t2, res.n_saturated, res.sum_t2, int(np.float32(res.gain).view(np.uint32))], np.uint64)


def run(V, ctx, c, install=False, t2=True, dense=True):
    """vk_local_thickness of a case: (rc, (t2 or None, dense or None, result)).  Outputs start from a pattern the call must overwrite."""
    N = V.native
    req, vb = request(c, install)
    arr = np.full(c.vol.shape, 0xABABABAB, np.uint32) if t2 else None
    out = np.full_like(np.ascontiguousarray(c.vol), 0x5A if c.kind == "u8" else 0) if dense else None
    res = N.VkThicknessResult(7, 7, 7, 7, 7.0)
    rc = N.lib().vk_local_thickness(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, arr.ctypes.data if arr is not None else None,
                                    out.ctypes.data if out is not None else None, C.byref(res))
    return rc, (arr, out, result_array(res))


assert TC.MAX_VOXELS == 48 * 40 * 33
