"""An independent numpy statement of vk_extract_isosurface's rule: marching tetrahedra over the cubes of a voxel box.
Whole-array np.float32 operations (each rounded once), the permutations from itertools, their parity from their inversions, the table parsed
from the text of the rule; the triangles are produced tetrahedron by tetrahedron and mask by mask and then sorted into the stated order
(cube, k, table position), so nothing of the C restatement's loop structure is shared."""
import itertools

import numpy as np

SCALE = {"u8": 255.0, "u16": 65535.0, "f16": 1.0}
TABLE_TEXT = """
1: (01,02,03)
2: (01,13,12)
3: (02,03,13) (02,13,12)
4: (02,12,23)
5: (01,23,03) (01,12,23)
6: (01,13,23) (01,23,02)
7: (03,13,23)
8: (03,23,13)
9: (01,02,23) (01,23,13)
10: (01,23,12) (01,03,23)
11: (02,23,12)
12: (02,12,13) (02,13,03)
13: (01,12,13)
14: (01,03,02)
"""


def table():
    out = {}
    for line in TABLE_TEXT.strip().splitlines():
        mask, rest = line.split(":")
        out[int(mask)] = [tuple((int(e[0]), int(e[1])) for e in tri.strip("()").split(",")) for tri in rest.split()]
    return out


PERMS = list(itertools.permutations(range(3)))  # lexicographic


def is_odd(p):
    return sum(1 for i in range(3) for j in range(i + 1, 3) if p[i] > p[j]) % 2 == 1


def tet_vertices(k):
    """The four vertices of tetrahedron k as (i, j, k) offsets."""
    p = PERMS[k]
    v = [np.zeros(3, int)]
    v.append(v[0] + np.eye(3, dtype=int)[p[0]])
    v.append(v[1] + np.eye(3, dtype=int)[p[1]])
    v.append(np.ones(3, int))
    return v


def iso_k(kind, iso):
    return np.float32(iso) * np.float32(SCALE[kind]) if kind != "f16" else np.float32(iso)


def mesh(vol, kind, iso, box=None):
    """(n, 3, 3) float32: the triangles of the stored texels `vol` [nz, ny, nx] at threshold `iso` (sample values) over `box`."""
    nz, ny, nx = vol.shape
    (x0, y0, z0), (x1, y1, z1) = ((0, 0, 0), (nx, ny, nz)) if box is None else box
    cx, cy, cz = max(x1 - x0 - 1, 0), max(y1 - y0 - 1, 0), max(z1 - z0 - 1, 0)
    if cx * cy * cz == 0:
        return np.zeros((0, 3, 3), np.float32)
    V = vol.astype(np.float32)
    ik = iso_k(kind, iso)
    dims = np.array([nx, ny, nz], np.float32)

    def corner(o):
        return V[z0 + o[2]:z0 + o[2] + cz, y0 + o[1]:y0 + o[1] + cy, x0 + o[0]:x0 + o[0] + cx]

    corners = {o: corner(o) for o in itertools.product((0, 1), repeat=3)}
    finite = np.ones((cz, cy, cx), bool)
    n_in = np.zeros((cz, cy, cx), int)
    with np.errstate(invalid="ignore"):
        for c in corners.values():
            finite &= np.isfinite(c)
            n_in += c >= ik
    live = finite & (n_in > 0) & (n_in < 8)
    zz, yy, xx = np.meshgrid(np.arange(cz), np.arange(cy), np.arange(cx), indexing="ij")
    cube_id = (zz * cy + yy) * cx + xx
    low = np.stack([xx + x0, yy + y0, zz + z0], -1)
    T = table()
    tris, keys = [], []
    for k in range(6):
        verts = tet_vertices(k)
        vals = [corners[tuple(v)] for v in verts]
        with np.errstate(invalid="ignore"):
            mask = sum((vals[i] >= ik).astype(int) << i for i in range(4))
        for m, rows in T.items():
            sel = live & (mask == m)
            if not sel.any():
                continue
            for t, tri in enumerate(rows):
                order = (tri[0], tri[2], tri[1]) if is_odd(PERMS[k]) else tri
                pts = []
                for a, b in order:
                    vA, vB = vals[a][sel], vals[b][sel]
                    f = (ik - vA) / (vB - vA)
                    A = (low[sel] + verts[a]).astype(np.float32)
                    moves = verts[b] > verts[a]
                    pts.append(((A + np.float32(0.5)) + np.where(moves[None, :], f[:, None], np.float32(0.0)).astype(np.float32)) / dims)
                tris.append(np.stack(pts, 1).astype(np.float32))
                cid = cube_id[sel]
                keys.append(np.stack([cid, np.full_like(cid, k), np.full_like(cid, t)], 1))
    if not tris:
        return np.zeros((0, 3, 3), np.float32)
    tris, keys = np.concatenate(tris), np.concatenate(keys)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return tris[order]
