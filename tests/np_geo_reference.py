"""vk_geodesic_distance in numpy, written another way than tests/geo_restatement.c: no queue and no order of settling, but sweeps of
the whole array -- every voxel of the set takes the minimum of itself and its shifted neighbours plus the step's cost, offset after
offset, until a whole sweep changes nothing.  The saturating step is monotone and commutes with min, so the sweeps end in the rule's
fixed point.  Nothing of the library is used; the integer square root of a step cost is written out below."""
import numpy as np

import np_label_reference as NL

G_INF, G_FAR = 0xFFFFFFFF, 0xFFFFFFFE


def isqrt(v):
    """The largest r with r r <= v, by Newton's iteration on integers."""
    if v < 2:
        return v
    r = 1 << ((v.bit_length() + 1) // 2)
    while True:
        t = (r + v // r) // 2
        if t >= r:
            return r
        r = t


def step_cost(spacing, dx, dy, dz):
    return isqrt(((spacing[0] * dx) ** 2 + (spacing[1] * dy) ** 2 + (spacing[2] * dz) ** 2) * 65536)


def face_mask(shape3, box, mask):
    """bool [nz, ny, nx]: the voxels of the box whose coordinate is the box's first or last index on a face of `mask`."""
    nz, ny, nx = shape3
    x0, y0, z0, x1, y1, z1 = box if box is not None else (0, 0, 0, nx, ny, nz)
    m = np.zeros(shape3, bool)
    if x1 <= x0 or y1 <= y0 or z1 <= z0:
        return m
    if mask & 1: m[:, :, x0] = True
    if mask & 2: m[:, :, x1 - 1] = True
    if mask & 4: m[:, y0, :] = True
    if mask & 8: m[:, y1 - 1, :] = True
    if mask & 16: m[z0, :, :] = True
    if mask & 32: m[z1 - 1, :, :] = True
    return m & NL.box_mask(shape3, box)


def distances(s, a, spacing, conn):
    """int64 [nz, ny, nx]: g over the set s from the source set a (a subset of s); G_INF where unreached and off s."""
    g = np.where(a, 0, G_INF).astype(np.int64)
    steps = [(dz, dy, dx, step_cost(spacing, dx, dy, dz)) for dz, dy, dx in NL.offsets(conn)]
    nz, ny, nx = s.shape
    while True:
        before = g.copy()
        for dz, dy, dx, w in steps:
            (zd, zs), (yd, ys), (xd, xs) = NL._shifted(nz, dz), NL._shifted(ny, dy), NL._shifted(nx, dx)
            src = g[zs, ys, xs]
            cand = np.where(src == G_INF, G_INF, np.minimum(src + w, G_FAR))
            dst = g[zd, yd, xd]
            np.minimum(dst, np.where(s[zd, yd, xd], cand, G_INF), out=dst)
        if (g == before).all():
            return g


def apply(vol, kind, lo, hi, conn, spacing, sources, targets, seeds, gain, fill_out, fill_unreached, box):
    """(g uint32 [nz, ny, nx], dense, result uint64 [9]: n_foreground, n_sources, n_reached, n_saturated, n_target_reached, sum_g, max_g,
    target_min, the bits of the gain used)."""
    v = np.asarray(vol)
    s = NL.foreground(v, kind, lo, hi, box)
    picked = face_mask(v.shape, box, sources)
    for x, y, z in seeds:
        picked[z, y, x] = True
    a = s & picked
    g = distances(s, a, spacing, conn)
    reached = s & (g != G_INF)
    on_target = reached & face_mask(v.shape, box, targets)
    top = int(g[reached].max()) if reached.any() else 0
    k = np.float32(gain)
    if k == 0:
        k = np.float32(1.0) / np.float32(np.uint32(top)) if top else np.float32(0.0)
    w = g.astype(np.uint32).astype(np.float32) * k
    dense = np.where(reached, NL.fill_bits(w, kind), np.where(s, np.full(v.shape, NL.fill_bits(fill_unreached, kind), v.dtype), np.full(v.shape, NL.fill_bits(fill_out, kind), v.dtype))).astype(v.dtype)
    result = np.array([s.sum(), a.sum(), reached.sum(), (reached & (g == G_FAR)).sum(), on_target.sum(), int(g[reached].astype(np.uint64).sum()), top,
                       int(g[on_target].min()) if on_target.any() else G_INF, int(np.float32(k).view(np.uint32))], np.uint64)
    return g.astype(np.uint32), dense, result
