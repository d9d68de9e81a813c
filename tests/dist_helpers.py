"""Shared by the distance-transform tests: the C restatement (tests/dist_restatement.c), a case through it and through the numpy reference,
the comparison of two results, and a case as the library's request.  Layouts and uploads are the label tests' (label_helpers)."""
import ctypes as C
import os
import subprocess

import numpy as np

import dist_cases as DC
import label_helpers as LH
import np_dist_reference as ND

ROOT = LH.ROOT
OP = {name: k for k, name in enumerate(ND.OPS)}


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libdist_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "dist_restatement.c"), "-lm"], check=True)
    L = C.CDLL(so)
    L.dist_restate.restype = C.c_int
    return L


def restate(L, vol, kind, lo, hi, op, spacing, radius, fill_in, fill_out, box=None):
    """(d2 or None, dense or None, result uint64 [5]); None when the restatement refuses the volume for overflow."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    b = np.array(box if box is not None else LH.whole(v), np.uint32)
    sp = np.array(spacing, np.uint32)
    d2, dense, result = np.zeros(v.shape, np.uint32), np.zeros_like(v), np.zeros(5, np.uint64)
    rc = L.dist_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(LH.FMT[kind]), C.c_float(lo), C.c_float(hi), C.c_int(OP[op]),
                        C.c_void_p(sp.ctypes.data), C.c_float(radius), C.c_float(fill_in), C.c_float(fill_out), C.c_void_p(b.ctypes.data), C.c_void_p(d2.ctypes.data),
                        C.c_void_p(dense.ctypes.data), C.c_void_p(result.ctypes.data))
    if rc == -2:
        return None
    assert rc == 0, rc
    return (d2, None, result) if op in ("outside", "inside") else (None, dense, result)


def restate_case(L, c):
    return restate(L, c.vol, c.kind, c.lo, c.hi, c.op, c.spacing, c.radius, c.fill_in, c.fill_out, c.box)


def reference_case(c, d2=ND.d2_to):
    return ND.apply(c.vol, c.kind, c.lo, c.hi, c.op, c.spacing, c.radius, c.fill_in, c.fill_out, c.box, d2)


def differences(got, ref):
    """Where two results (d2, dense, result) differ, in words (empty: bitwise equal)."""
    if got is None or ref is None:
        return "" if got is None and ref is None else "one of the two refuses the case"
    out = []
    for name, g, r in zip(("d2", "dense", "result"), got, ref):
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
    """A case as the library's request (with VK_DIST_CLIP_BOX where the case's box is the clip box) and its box argument."""
    from vokselis_amd import _native as N
    from vokselis_amd.distance import distance_request

    req = distance_request(c.lo, c.hi, op=c.op, radius=c.radius, spacing=c.spacing, fill_in=c.fill_in, fill_out=c.fill_out, install=install,
                           box="clip" if c.clip is not None else None)
    vb = N.VkVoxelBox(*c.box) if c.box is not None and c.clip is None else None
    return req, vb


def result_array(res):
    return np.array([res.n_foreground, res.n_result, res.n_added, res.n_removed, res.max_d2], np.uint64)


def run(V, ctx, c, install=False):
    """vk_distance_transform of a case: (rc, (d2 or None, dense or None, result)).  Outputs start from a pattern the call must overwrite."""
    N = V.native
    req, vb = request(c, install)
    morph = c.op in DC.MORPH
    d2 = None if morph else np.full(c.vol.shape, 0xABABABAB, np.uint32)
    dense = np.zeros_like(np.ascontiguousarray(c.vol)) if morph else None
    res = N.VkDistanceResult(7, 7, 7, 7, 7, 7)
    rc = N.lib().vk_distance_transform(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, d2.ctypes.data if d2 is not None else None,
                                       dense.ctypes.data if dense is not None else None, C.byref(res))
    return rc, (d2, dense, result_array(res))


assert DC.MAX_VOXELS == 48 * 40 * 33
