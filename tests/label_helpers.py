"""Shared by the connected-components tests: the C restatement (tests/label_restatement.c), a case through it and through the numpy
reference (each computed once per case), the comparison of two results, the layouts of each format with their upload, and a case as the
library's request."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_cases as LC
import np_label_reference as NL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"u8": 0, "f16": 1, "u16": 3}
KEEP = {"all": 0, "largest": 1, "min_size": 2, "seeds": 3}
LAYOUTS = {"u8": ("LINEAR", "PACKED", "PACKED_PAIRS"), "f16": ("LINEAR", "PACKED"), "u16": ("LINEAR", "PACKED")}


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "liblabel_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "label_restatement.c"), "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.label_restate.restype = C.c_int
    return L


def whole(vol):
    return (0, 0, 0, vol.shape[2], vol.shape[1], vol.shape[0])


def restate(L, vol, kind, lo, hi, conn, box=None, keep="all", count=0, seeds=(), invert=False, fill=0.0, cap=None):
    """(labels uint32 [nz, ny, nx], table uint64 [min(n, cap), 8], result uint64 [4], dense in the volume's dtype)."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    b = np.array(box if box is not None else whole(v), np.uint32)
    s = np.array(seeds, np.uint32).reshape(-1, 3) if len(seeds) else np.zeros((1, 3), np.uint32)
    labels, dense, result = np.zeros(v.shape, np.uint32), np.zeros_like(v), np.zeros(4, np.uint64)
    room = v.size if cap is None else cap
    table = np.zeros((max(room, 1), 8), np.uint64)
    rc = L.label_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(FMT[kind]), C.c_float(lo), C.c_float(hi), C.c_uint32(conn),
                         C.c_void_p(b.ctypes.data), C.c_int(KEEP[keep]), C.c_uint64(count), C.c_uint32(len(seeds)), C.c_void_p(s.ctypes.data), C.c_int(1 if invert else 0),
                         C.c_float(fill), C.c_void_p(labels.ctypes.data), C.c_void_p(table.ctypes.data), C.c_uint64(room), C.c_void_p(result.ctypes.data), C.c_void_p(dense.ctypes.data))
    assert rc == 0, rc
    return labels, table[:min(int(result[0]), room)].copy(), result, dense


def restate_case(L, c, cap=None):
    return restate(L, c.vol, c.kind, c.lo, c.hi, c.conn, c.box, c.keep, c.count, c.seeds, c.invert, c.fill, cap)


def reference_case(c):
    return NL.apply(c.vol, c.kind, c.lo, c.hi, c.conn, c.box, c.keep, c.count, c.seeds, c.invert, c.fill)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def differences(got, ref):
    """Where two results (labels, table, result, dense) differ, in words (empty: bitwise equal)."""
    out = []
    for name, g, r in zip(("labels", "table", "result", "dense"), got, ref):
        if g is None or r is None:
            continue
        g, r = raw(g), raw(r)
        if g.shape != r.shape or g.dtype != r.dtype:
            out.append(f"{name}: shape / dtype {g.shape} {g.dtype} != {r.shape} {r.dtype}")
        elif (g != r).any():
            at = np.argwhere(g != r)[0]
            out.append(f"{name}: {int((g != r).sum())} of {g.size} differ, first at {tuple(int(v) for v in at)} (array order): {g[tuple(at)]} != {r[tuple(at)]}")
    return "; ".join(out)


def upload(V, ctx, vol, kind, layout):
    kw = dict(fmt=V.FMT_R16_UNORM) if kind == "u16" else {}
    return V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout), **kw)


def request(c, install=False):
    """A case as the library's request (with VK_LABEL_CLIP_BOX where the case's box is the clip box) and its box argument."""
    from vokselis_amd import _native as N
    from vokselis_amd.label import label_request

    req = label_request(c.lo, c.hi, connectivity=c.conn, box="clip" if c.clip is not None else None, keep=c.keep, count=c.count, seeds=c.seeds, invert=c.invert, fill=c.fill,
                        install=install)
    vb = N.VkVoxelBox(*c.box) if c.box is not None and c.clip is None else None
    return req, vb


def table_array(components, n):
    """n vk_component as the uint64 [n, 8] the references use."""
    return np.array([[components[k].n_voxels, components[k].first, components[k].box.x0, components[k].box.y0, components[k].box.z0, components[k].box.x1, components[k].box.y1,
                      components[k].box.z1] for k in range(n)], np.uint64).reshape(n, 8)


def run(V, ctx, c, cap=None, install=False, dense=True, labels=True):
    """vk_label_components of a case: (rc, (labels, table, result, dense))."""
    N = V.native
    req, vb = request(c, install)
    lab = np.full(c.vol.shape, 0xABABABAB, np.uint32) if labels else None
    out = np.zeros_like(np.ascontiguousarray(c.vol)) if dense else None
    room = c.vol.size if cap is None else cap
    comps = (N.VkComponent * max(room, 1))()
    res = N.VkLabelResult()
    rc = N.lib().vk_label_components(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, lab.ctypes.data if labels else None, comps, room,
                                     out.ctypes.data if dense else None, C.byref(res))
    result = np.array([res.n_components, res.n_foreground, res.n_kept_components, res.n_kept_voxels], np.uint64)
    return rc, (lab, table_array(comps, min(int(res.n_components), room)), result, out)


assert LC.MAX_VOXELS == 48 * 40 * 33
