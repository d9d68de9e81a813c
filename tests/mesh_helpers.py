"""Shared by the mesh tests: the C restatement (tests/mesh_restatement.c, built with -ffp-contract=off), a case through it, and the topology
of a triangle soup -- welding by bit pattern, closedness and orientation from the directed edges, Euler characteristic, signed volume."""
import ctypes as C
import os
import subprocess

import numpy as np

import np_mesh_reference as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"u8": 0, "f16": 1, "u16": 3}
N_KINDS = 4 + 16 * 6  # mesh_restatement.c's kind counters: non-finite cubes, all-inside cubes, f == 0, f == 1, then [k][mask]
LAYOUTS = {"u8": ("LINEAR", "PACKED", "PACKED_PAIRS"), "f16": ("LINEAR", "PACKED"), "u16": ("LINEAR", "PACKED")}


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libmesh_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "mesh_restatement.c"), "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.mesh_restate.restype = C.c_uint64
    return L


def restate_k(L, vol, kind, iso_k, box=None, cap=None, kinds=None):
    """The restatement's triangles (n, 3, 3) at the threshold iso_k on the kernel's scale; cap: at most that many (the count is returned too)."""
    v = np.ascontiguousarray(vol)
    raw = v.view(np.uint16) if kind == "f16" else v
    nz, ny, nx = v.shape
    (x0, y0, z0), (x1, y1, z1) = ((0, 0, 0), (nx, ny, nz)) if box is None else box
    b = np.array([x0, y0, z0, x1, y1, z1], np.uint32)
    kp = C.c_void_p(kinds.ctypes.data) if kinds is not None else None
    args = (C.c_void_p(raw.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(FMT[kind]), C.c_void_p(b.ctypes.data), C.c_float(float(iso_k)))
    n = int(L.mesh_restate(*args, None, C.c_uint64(0), None))
    m = n if cap is None else min(n, cap)
    out = np.zeros((m, 3, 3), np.float32)
    n2 = int(L.mesh_restate(*args, C.c_void_p(out.ctypes.data), C.c_uint64(m), kp))
    assert n2 == n
    return out


def restate(L, vol, kind, iso, box=None, cap=None, kinds=None):
    return restate_k(L, vol, kind, NM.iso_k(kind, iso), box, cap, kinds)


def restate_case(L, c, kinds=None):
    return restate(L, c.vol, c.kind, c.iso, c.box, None, kinds)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def upload(V, ctx, vol, kind, layout):
    kw = dict(fmt=V.FMT_R16_UNORM) if kind == "u16" else {}
    return V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout), **kw)


# ---- topology ---------------------------------------------------------------------------------------------------------------------
def weld(tris):
    """(vertices [m, 3] f32, faces [n, 3]): vertices with the same bit pattern become one."""
    bits = np.ascontiguousarray(tris, np.float32).reshape(-1, 3).view(np.uint32)
    uniq, inv = np.unique(bits, axis=0, return_inverse=True)
    return uniq.view(np.float32), inv.reshape(-1, 3)


def edge_report(faces):
    """(closed, oriented): every undirected edge in exactly two triangles; those two run it in opposite directions (every directed edge once)."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    und = np.sort(e, axis=1)
    _, cnt = np.unique(und, axis=0, return_counts=True)
    _, dcnt = np.unique(e, axis=0, return_counts=True)
    return bool((cnt == 2).all()), bool((dcnt == 1).all())


def euler(verts, faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return len(verts) - len(np.unique(e, axis=0)) + len(faces)


def signed_volume(tris):
    t = tris.astype(np.float64)
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


def normals(tris):
    t = tris.astype(np.float64)
    return np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
