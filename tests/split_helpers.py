"""Shared by the split tests: the C restatement (tests/split_restatement.c), a case through it and through the numpy reference, a case as
the library's request, and the call on a context.  The comparison of two results, the layouts and the upload are label_helpers'."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_helpers as LH
import np_split_reference as NS
import split_cases as SC

ROOT = LH.ROOT
RESULT_FIELDS = ("n_regions", "n_foreground", "n_markers", "n_marker_voxels", "n_residue_regions", "n_residue_voxels", "n_cut", "rounds")


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libsplit_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "split_restatement.c"), "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.split_restate.restype = C.c_int
    return L


def restate(L, vol, kind, lo, hi, conn, radius, box=None, spacing=(1, 1, 1), fill_out=0.0, cap=None):
    """(labels uint32 [nz, ny, nx], table uint64 [min(N, cap), 8], result uint64 [8], dense in the volume's dtype, g uint32)."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    b = np.array(box if box is not None else LH.whole(v), np.uint32)
    s = np.array(spacing, np.uint32)
    labels, dense, result, g = np.zeros(v.shape, np.uint32), np.zeros_like(v), np.zeros(8, np.uint64), np.zeros(v.shape, np.uint32)
    room = v.size if cap is None else cap
    table = np.zeros((max(room, 1), 8), np.uint64)
    rc = L.split_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(LH.FMT[kind]), C.c_float(lo), C.c_float(hi), C.c_uint32(conn),
                         C.c_void_p(b.ctypes.data), C.c_void_p(s.ctypes.data), C.c_float(radius), C.c_float(fill_out), C.c_void_p(labels.ctypes.data), C.c_void_p(table.ctypes.data),
                         C.c_uint64(room), C.c_void_p(result.ctypes.data), C.c_void_p(dense.ctypes.data), C.c_void_p(g.ctypes.data))
    assert rc == 0, rc
    return labels, table[:min(int(result[0]), room)].copy(), result, dense, g


def restate_case(L, c, cap=None):
    return restate(L, c.vol, c.kind, c.lo, c.hi, c.conn, c.radius, c.box, c.spacing, c.fill_out, cap)


def reference_case(c):
    return NS.apply(c.vol, c.kind, c.lo, c.hi, c.conn, c.box, c.spacing, c.radius, c.fill_out)


def request(c, install=False):
    """A case as the library's request (with VK_SPLIT_CLIP_BOX where the case's box is the clip box) and its box argument."""
    from vokselis_amd import _native as N
    from vokselis_amd.split import split_request

    req = split_request(c.lo, c.hi, radius=c.radius, spacing=c.spacing, connectivity=c.conn, box="clip" if c.clip is not None else None, fill_out=c.fill_out, install=install)
    vb = N.VkVoxelBox(*c.box) if c.box is not None and c.clip is None else None
    return req, vb


def result_array(res):
    return np.array([getattr(res, f) for f in RESULT_FIELDS], np.uint64)


def run(V, ctx, c, cap=None, install=False, dense=True, labels=True):
    """vk_split_components of a case: (rc, (labels, table, result, dense))."""
    N = V.native
    req, vb = request(c, install)
    lab = np.full(c.vol.shape, 0xABABABAB, np.uint32) if labels else None
    out = np.zeros_like(np.ascontiguousarray(c.vol)) if dense else None
    room = c.vol.size if cap is None else cap
    comps = (N.VkComponent * max(room, 1))()
    res = N.VkSplitResult()
    rc = N.lib().vk_split_components(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, lab.ctypes.data if labels else None, comps, room,
                                     out.ctypes.data if dense else None, C.byref(res))
    return rc, (lab, LH.table_array(comps, min(int(res.n_regions), room)), result_array(res), out)


assert SC.MAX_VOXELS == 70 * 35 * 19
