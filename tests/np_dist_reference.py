"""vk_distance_transform restated in numpy from the rule in include/vokselis_hip.h.  D2(A, v) is taken literally where the volume is small
(brute: every voxel against every voxel of A) and axis by axis otherwise (d2_to: along each axis a whole-array minimum over all pairs of
entries of a line, z first) -- the two are held together by the CPU tests.  dil and ero are the header's two definitions, composed as it
composes them.  Shares nothing with the library's line function or with the C restatement's loops."""
import math

import numpy as np

import np_label_reference as NL

INF = 0xFFFFFFFF
OPS = ("outside", "inside", "dilate", "erode", "close", "open")
_NONE = np.int64(1) << 62


def fits(dims, spacing):
    """The header's bound: sum_c (spacing[c] (n_c - 1))^2 <= 0xFFFFFFFE (Python integers)."""
    return sum((int(s) * (int(n) - 1)) ** 2 for s, n in zip(spacing, dims)) <= 0xFFFFFFFE


def d2_to(a, spacing):
    """uint32 [nz, ny, nx]: D2(A, v) for the bool array a; INF everywhere when a is empty.  spacing: (sx, sy, sz)."""
    g = np.where(a, np.int64(0), _NONE)
    for axis, w in ((0, spacing[2]), (1, spacing[1]), (2, spacing[0])):
        n = g.shape[axis]
        idx = np.arange(n, dtype=np.int64)
        cost = (int(w) * (idx[:, None] - idx[None, :])) ** 2          # [i, j]
        line = np.moveaxis(g, axis, -1)                                # [..., j]
        out = np.empty_like(line)
        for i in range(n):                                             # min over j of g(j) + (w (i - j))^2
            out[..., i] = (line + cost[i]).min(axis=-1)
        g = np.moveaxis(out, -1, axis)
    return np.where(g >= _NONE, INF, g).astype(np.uint32)


def brute(a, spacing):
    """The same by the definition: every voxel against every voxel of A (small volumes)."""
    z, y, x = (c.ravel().astype(np.int64) for c in np.indices(a.shape))
    sel = np.flatnonzero(a.ravel())
    if not len(sel):
        return np.full(a.shape, INF, np.uint32)
    sx, sy, sz = (int(s) for s in spacing)
    out = np.empty(a.size, np.uint32)
    for k in range(0, a.size, 1024):  # (in slabs of voxels: the table of all pairs would not fit)
        v = slice(k, k + 1024)
        d = (sx * (x[v, None] - x[sel][None, :])) ** 2 + (sy * (y[v, None] - y[sel][None, :])) ** 2 + (sz * (z[v, None] - z[sel][None, :])) ** 2
        out[v] = d.min(axis=1)
    return out.reshape(a.shape)


def r2_of(radius):
    return int(math.floor(float(np.float32(radius)) * float(np.float32(radius))))


def dil(a, spacing, r2, d2=d2_to):
    return d2(a, spacing).astype(np.int64) <= r2 if a.any() else np.zeros(a.shape, bool)


def ero(a, spacing, r2, d2=d2_to):
    return d2(~a, spacing).astype(np.int64) > r2 if not a.all() else np.ones(a.shape, bool)


def morph(s, op, spacing, r2, d2=d2_to):
    if op == "dilate":
        return dil(s, spacing, r2, d2)
    if op == "erode":
        return ero(s, spacing, r2, d2)
    if op == "close":
        return ero(dil(s, spacing, r2, d2), spacing, r2, d2)
    if op == "open":
        return dil(ero(s, spacing, r2, d2), spacing, r2, d2)
    raise ValueError(op)


def apply(vol, kind, lo, hi, op, spacing, radius, fill_in, fill_out, box, d2=d2_to):
    """(d2 uint32 [nz, ny, nx] or None, dense or None, result uint64 [5]: n_foreground, n_result, n_added, n_removed, max_d2); None when
    the header refuses the volume for overflow."""
    v = np.asarray(vol)
    if not fits(tuple(reversed(v.shape)), spacing):
        return None
    s = NL.foreground(v, kind, lo, hi, box)
    if op in ("outside", "inside"):
        d = d2(s if op == "outside" else ~s, spacing)
        finite = d[d != INF]
        return d, None, np.array([s.sum(), s.sum(), 0, 0, int(finite.max()) if finite.size else 0], np.uint64)
    m = morph(s, op, spacing, r2_of(radius), d2)
    dense = np.where(m & ~s, np.full(v.shape, NL.fill_bits(fill_in, kind), v.dtype), np.where(s & ~m, np.full(v.shape, NL.fill_bits(fill_out, kind), v.dtype), v))
    return None, dense, np.array([s.sum(), m.sum(), (m & ~s).sum(), (s & ~m).sum(), 0], np.uint64)
