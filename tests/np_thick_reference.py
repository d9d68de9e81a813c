"""vk_local_thickness in numpy, written another way than tests/thick_restatement.c: not ball by ball but level by level.  For each
distinct value d of Dc, descending, the voxels of S that no larger level has claimed and that lie within d2 < d of the set { Dc == d }
take d -- a voxel's T2 is the largest Dc among the balls that hold it, and the levels arrive largest first.  Every distance comes from
np_dist_reference (an envelope-free minimum along lines), none from the library."""
import math

import numpy as np

import np_dist_reference as ND
import np_label_reference as NL


def cap_of(max_radius):
    return int(math.floor(float(np.float32(max_radius)) * float(np.float32(max_radius))))


def capped_distance(s, spacing, cap):
    """int64 [nz, ny, nx]: Dc = min(D2(not S, .), C); INF (S is the whole volume) caps to C; 0 off S."""
    d = ND.d2_to(~s, spacing).astype(np.int64) if not s.all() else np.full(s.shape, cap, np.int64)
    return np.where(s, np.minimum(d, cap), 0)


def t2_of(s, spacing, cap):
    dc = capped_distance(s, spacing, cap)
    t2 = np.zeros(s.shape, np.int64)
    free = s.copy()
    for d in sorted((int(v) for v in np.unique(dc[s])), reverse=True):
        if not free.any():
            break
        near = ND.d2_to(dc == d, spacing).astype(np.int64) < d
        take = free & near
        t2[take] = d
        free &= ~take
    assert not free.any()  # u = v always qualifies
    return t2.astype(np.uint32)


def apply(vol, kind, lo, hi, spacing, max_radius, gain, fill_out, box):
    """(t2 uint32 [nz, ny, nx], dense, result uint64 [5]: n_foreground, max_t2, n_saturated, sum_t2, the bits of the gain used); None
    when the header refuses the volume for overflow."""
    v = np.asarray(vol)
    if not ND.fits(tuple(reversed(v.shape)), spacing):
        return None
    s = NL.foreground(v, kind, lo, hi, box)
    cap = cap_of(max_radius)
    t2 = t2_of(s, spacing, cap)
    top = int(t2.max()) if t2.size else 0
    g = np.float32(gain)
    if g == 0:
        g = np.float32(1.0) / np.sqrt(np.float32(top)) if top else np.float32(0.0)
    w = np.sqrt(t2.astype(np.float32)) * g
    dense = np.where(s, NL.fill_bits(w, kind), np.full(v.shape, NL.fill_bits(fill_out, kind), v.dtype)).astype(v.dtype)
    result = np.array([s.sum(), top, (s & (t2 == cap)).sum(), t2.astype(np.uint64).sum(), int(np.float32(g).view(np.uint32))], np.uint64)
    return t2, dense, result
