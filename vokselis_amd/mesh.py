"""The triangles of Context.extract_isosurface (vk_extract_isosurface) as files and as an indexed mesh.  The library emits a triangle soup
whose shared vertices are bitwise equal -- a vertex is a function of its lattice edge alone -- so welding compares bit patterns, never
distances."""
from __future__ import annotations

import struct

import numpy as np


def _soup(tris) -> np.ndarray:
    t = np.ascontiguousarray(tris, np.float32)
    if t.ndim != 3 or t.shape[1:] != (3, 3):
        raise ValueError("triangles: an array of shape (n, 3, 3)")
    return t


def weld(tris):
    """(vertices, faces): vertices float32 (m, 3), each bit pattern once, in order of first use; faces int64 (n, 3) into them, triangle
    for triangle in the order given.  -0 and +0 are different patterns, as are two NaNs of different payload."""
    t = _soup(tris)
    bits = t.reshape(-1, 3).view(np.uint32)
    if len(bits) == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    uniq, first, inv = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")       # unique rows by first use
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return uniq[order].view(np.float32), rank[inv.reshape(-1)].reshape(-1, 3)


def write_stl(path, tris, scale=(1.0, 1.0, 1.0)) -> int:
    """Binary STL: 80 bytes of header, the count, and per triangle the facet normal and the three vertices as f32 and a zero attribute.
    scale multiplies the unit-cube coordinates per axis (the volume's physical extent), in double; the normal is formed in double from
    the scaled vertices and is (0, 0, 0) for a triangle without area.  Returns the triangle count."""
    t = _soup(tris).astype(np.float64) * np.asarray(scale, np.float64).reshape(1, 1, 3)
    if len(t) > 0xffffffff:
        raise ValueError("binary STL holds at most 2^32 - 1 triangles")
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    length = np.sqrt((n * n).sum(axis=1))
    n = np.where(length[:, None] > 0.0, n / np.where(length > 0.0, length, 1.0)[:, None], 0.0)
    rec = np.zeros(len(t), np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    rec["n"], rec["v"] = n, t
    with open(path, "wb") as f:
        f.write(b"vokselis_amd isosurface".ljust(80, b" "))
        f.write(struct.pack("<I", len(t)))
        f.write(rec.tobytes())
    return len(t)


def write_obj(path, tris) -> tuple:
    """Wavefront OBJ of the welded mesh: `v` lines with nine significant digits (an f32 survives the round trip), `f` lines 1-based.
    Returns (vertices, faces) written."""
    verts, faces = weld(tris)
    with open(path, "w") as f:
        f.write("# vokselis_amd isosurface: %d vertices, %d faces\n" % (len(verts), len(faces)))
        f.writelines("v %.9g %.9g %.9g\n" % tuple(float(c) for c in v) for v in verts)
        f.writelines("f %d %d %d\n" % tuple(int(i) + 1 for i in tri) for tri in faces)
    return len(verts), len(faces)
