"""Shared by the skeleton tests: the C restatement (tests/skel_restatement.c), a case through it and through the numpy reference, the
comparison of two results, a case as the library's request, and the topological numbers of a set (components of the set and of its
padded background, Euler characteristic).  Layouts and uploads are the label tests' (label_helpers)."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_helpers as LH
import np_label_reference as NL
import np_skel_reference as NS
import skel_cases as SC

ROOT = LH.ROOT
RESULT = ("n_foreground", "n_skeleton", "n_isolated", "n_end", "n_regular", "n_junction")
R_LINKS, R_ITERATIONS, R_CONVERGED, R_WORDS = 6, 19, 20, 21


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libskel_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "skel_restatement.c"), "-lm"], check=True)
    L = C.CDLL(so)
    L.skel_restate.restype = C.c_int
    return L


def restate(L, vol, kind, lo, hi, mode, max_iterations=0, fill_in=None, fill_out=0.0, box=None):
    """(classes uint8 [nz, ny, nx], dense, result uint64 [21]: RESULT, links[13], iterations, converged)."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    b = np.array(box if box is not None else LH.whole(v), np.uint32)
    cls, dense, result = np.zeros(v.shape, np.uint8), np.zeros_like(v), np.zeros(R_WORDS, np.uint64)
    rc = L.skel_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(LH.FMT[kind]), C.c_float(lo), C.c_float(hi), C.c_int(mode),
                        C.c_uint32(max_iterations), C.c_int(fill_in is not None), C.c_float(fill_in if fill_in is not None else 0.0), C.c_float(fill_out), C.c_void_p(b.ctypes.data),
                        C.c_void_p(cls.ctypes.data), C.c_void_p(dense.ctypes.data), C.c_void_p(result.ctypes.data))
    assert rc == 0, rc
    return cls, dense, result


def restate_case(L, c):
    return restate(L, c.vol, c.kind, c.lo, c.hi, c.mode, c.max_iterations, c.fill_in, c.fill_out, c.box)


def reference_case(c):
    return NS.apply(c.vol, c.kind, c.lo, c.hi, c.mode, c.max_iterations, c.fill_in, c.fill_out, c.box)


def differences(got, ref):
    """Where two results (classes, dense, result) differ, in words (empty: bitwise equal)."""
    out = []
    for name, g, r in zip(("classes", "dense", "result"), got, ref):
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
    """A case as the library's request (with VK_SKEL_CLIP_BOX where the case's box is the clip box) and its box argument."""
    from vokselis_amd import _native as N
    from vokselis_amd.skeleton import skeleton_request

    req = skeleton_request(c.lo, c.hi, mode=SC.MODE_NAME[c.mode], max_iterations=c.max_iterations, fill_in=c.fill_in, fill_out=c.fill_out, box="clip" if c.clip is not None else None,
                           install=install)
    vb = N.VkVoxelBox(*c.box) if c.box is not None and c.clip is None else None
    return req, vb


def result_array(res):
    return np.array([getattr(res, k) for k in RESULT] + list(res.links) + [res.iterations, res.converged], np.uint64)


def fresh_result(N):
    return N.VkSkeletonResult(7, 7, 7, 7, 7, 7, (C.c_uint64 * 13)(*([7] * 13)), 7, 7)


def run(V, ctx, c, install=False, classes=True, dense=True):
    """vk_skeletonize of a case: (rc, (classes or None, dense or None, result)).  Outputs start from a pattern the call must overwrite."""
    N = V.native
    req, vb = request(c, install)
    cls = np.full(c.vol.shape, 0xAB, np.uint8) if classes else None
    out = np.full_like(np.ascontiguousarray(c.vol), 0x5A if c.kind == "u8" else 0) if dense else None
    res = fresh_result(N)
    rc = N.lib().vk_skeletonize(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, cls.ctypes.data if cls is not None else None,
                                out.ctypes.data if out is not None else None, C.byref(res))
    return rc, (cls, out, result_array(res))


# ---- topology ---------------------------------------------------------------------------------------------------------------------------
def components(mask, conn):
    """How many components the set has under the connectivity."""
    if not mask.any():
        return 0
    return len(np.unique(NL.first_of_component(mask, conn)[mask]))


def background_components(mask):
    """The 6-components of the background after one layer of zeros around the array."""
    return components(~np.pad(mask, 1), 6)


def euler(mask):
    """Vertices - edges + faces - cubes of the cubical complex whose cubes are the set's voxels (closed unit cubes: the set 26-connected)."""
    p = np.pad(mask, 1)

    def spread(a, axes):
        for ax in axes:
            a = a | np.roll(a, 1, axis=ax)   # the padding keeps the roll from wrapping a set cell
        return a

    cubes = int(p.sum())
    faces = sum(int(spread(p, (ax,)).sum()) for ax in range(3))                        # a face normal to ax belongs to the cubes on either side
    edges = sum(int(spread(p, tuple(a for a in range(3) if a != ax)).sum()) for ax in range(3))   # an edge along ax to the four cubes around it
    vertices = int(spread(p, (0, 1, 2)).sum())
    return vertices - edges + faces - cubes


def topology(mask):
    return components(mask, 26), background_components(mask), euler(mask)


def snapshots(L, c, limit=400):
    """K after 0, 1, 2, ... iterations of the case (bool arrays), until an iteration deletes nothing."""
    ks = [NL.foreground(np.asarray(c.vol), c.kind, c.lo, c.hi, c.box), restate(L, c.vol, c.kind, c.lo, c.hi, c.mode, 1, None, 0.0, c.box)[0] != 0]
    while (ks[-1] != ks[-2]).any() and len(ks) < limit:
        ks.append(restate(L, c.vol, c.kind, c.lo, c.hi, c.mode, len(ks), None, 0.0, c.box)[0] != 0)
    return ks[:-1]


def tile_activity(ks):
    """From K after every iteration: (deleted[i][tz, ty, tx] whether iteration i + 1 deleted a voxel of the tile, active[i] whether the
    tile runs in iteration i + 1: it holds a voxel of S (i = 0), or it or a tile around it deleted something in the iteration before)."""
    tx, ty, tz = SC.TILE
    nz, ny, nx = ks[0].shape

    def per_tile(m):
        p = np.zeros((-(-nz // tz) * tz, -(-ny // ty) * ty, -(-nx // tx) * tx), bool)
        p[:nz, :ny, :nx] = m
        return p.reshape(p.shape[0] // tz, tz, p.shape[1] // ty, ty, p.shape[2] // tx, tx).any(axis=(1, 3, 5))

    def around(t):
        p = np.pad(t, 1)
        out = np.zeros_like(t)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    out |= p[dz:dz + t.shape[0], dy:dy + t.shape[1], dx:dx + t.shape[2]]
        return out

    deleted = [per_tile(a & ~b) for a, b in zip(ks, ks[1:])]
    active = [per_tile(ks[0])] + [around(d) for d in deleted]
    return deleted, active


assert SC.MAX_VOXELS == 64000
