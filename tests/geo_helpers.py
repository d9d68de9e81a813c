"""Shared by the geodesic-distance tests: the C restatement (tests/geo_restatement.c), a case through it and through the numpy reference,
the comparison of two results, and a case as the library's request.  Layouts and uploads are the label tests' (label_helpers)."""
import ctypes as C
import os
import subprocess

import numpy as np

import geo_cases as GC
import label_helpers as LH
import np_geo_reference as NG

ROOT = LH.ROOT
RESULT = ("n_foreground", "n_sources", "n_reached", "n_saturated", "n_target_reached", "sum_g", "max_g", "target_min")


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libgeo_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "geo_restatement.c"), "-lm"], check=True)
    L = C.CDLL(so)
    L.geo_restate.restype = C.c_int
    return L


def restate(L, vol, kind, lo, hi, conn, spacing, sources, targets, seeds=(), gain=0.0, fill_out=0.0, fill_unreached=0.0, box=None):
    """(g uint32 [nz, ny, nx], dense, result uint64 [9]: RESULT and the bits of the gain used)."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    b = np.array(box if box is not None else LH.whole(v), np.uint32)
    sp = np.array(spacing, np.uint32)
    sd = np.array([c for s in seeds for c in s] or [0], np.uint32)
    g, dense, result = np.zeros(v.shape, np.uint32), np.zeros_like(v), np.zeros(9, np.uint64)
    rc = L.geo_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(LH.FMT[kind]), C.c_float(lo), C.c_float(hi), C.c_uint32(conn),
                       C.c_void_p(sp.ctypes.data), C.c_uint32(sources), C.c_uint32(targets), C.c_uint32(len(seeds)), C.c_void_p(sd.ctypes.data), C.c_float(gain), C.c_float(fill_out),
                       C.c_float(fill_unreached), C.c_void_p(b.ctypes.data), C.c_void_p(g.ctypes.data), C.c_void_p(dense.ctypes.data), C.c_void_p(result.ctypes.data))
    assert rc == 0, rc
    return g, dense, result


def restate_case(L, c):
    return restate(L, c.vol, c.kind, c.lo, c.hi, c.conn, c.spacing, c.sources, c.targets, c.seeds, c.gain, c.fill_out, c.fill_unreached, c.box)


def reference_case(c):
    return NG.apply(c.vol, c.kind, c.lo, c.hi, c.conn, c.spacing, c.sources, c.targets, c.seeds, c.gain, c.fill_out, c.fill_unreached, c.box)


def differences(got, ref):
    """Where two results (g, dense, result) differ, in words (empty: bitwise equal)."""
    out = []
    for name, g, r in zip(("g", "dense", "result"), got, ref):
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
    """A case as the library's request (with VK_GEO_CLIP_BOX where the case's box is the clip box) and its box argument."""
    from vokselis_amd import _native as N
    from vokselis_amd.geodesic import geodesic_request

    req = geodesic_request(c.lo, c.hi, sources=(), seeds=c.seeds, targets=(), connectivity=c.conn, spacing=c.spacing, gain=c.gain, fill_out=c.fill_out, fill_unreached=c.fill_unreached,
                           box="clip" if c.clip is not None else None, install=install)
    req.source_faces, req.target_faces = c.sources, c.targets
    vb = N.VkVoxelBox(*c.box) if c.box is not None and c.clip is None else None
    return req, vb


def result_array(res):
    return np.array([getattr(res, k) for k in RESULT] + [int(np.float32(res.gain).view(np.uint32))], np.uint64)


def fresh_result(N):
    return N.VkGeodesicResult(7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7)


def run(V, ctx, c, install=False, g=True, dense=True):
    """vk_geodesic_distance of a case: (rc, (g or None, dense or None, result)).  Outputs start from a pattern the call must overwrite."""
    N = V.native
    req, vb = request(c, install)
    arr = np.full(c.vol.shape, 0xABABABAB, np.uint32) if g else None
    out = np.full_like(np.ascontiguousarray(c.vol), 0x5A if c.kind == "u8" else 0) if dense else None
    res = fresh_result(N)
    rc = N.lib().vk_geodesic_distance(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, arr.ctypes.data if arr is not None else None,
                                      out.ctypes.data if out is not None else None, C.byref(res))
    return rc, (arr, out, result_array(res))


def tile_of(voxel):
    return tuple(int(v) // t for v, t in zip(voxel, GC.TILE))


def tile_crossings(path):
    """How often a path (n, 3) steps from one tile into another."""
    tiles = [tile_of(p) for p in path]
    return sum(a != b for a, b in zip(tiles, tiles[1:]))


assert GC.MAX_VOXELS == 64000
