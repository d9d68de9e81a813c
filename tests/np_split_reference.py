"""vk_split_components restated in numpy from the rule in include/vokselis_hip.h, by its definitions: K from the distance reference's
erosion; g as the length of the shortest path from K inside S -- g = min(g, 1 + the smallest g among the neighbours), relaxed in whole-array
sweeps until nothing changes, in no particular order --; a(v) level by level, as the minimum of a over the neighbours one step closer; the
unreached voxels through the label reference; numbering, table and cut in whole-array operations.  Shares nothing with the library or with
the C restatement's breadth-first rounds."""
import numpy as np

import np_dist_reference as ND
import np_label_reference as NL

FAR = np.int64(1) << 40


def _neighbour_min(a, conn, fill):
    """[nz, ny, nx]: the smallest a among each voxel's neighbours (fill where it has none)."""
    m = np.full(a.shape, fill, a.dtype)
    for d in NL.offsets(conn):
        (dz, sz), (dy, sy), (dx, sx) = (NL._shifted(a.shape[k], d[k]) for k in range(3))
        m[dz, dy, dx] = np.minimum(m[dz, dy, dx], a[sz, sy, sx])
    return m


def steps(S, K, conn):
    """int64 [nz, ny, nx]: g, FAR where it is not finite (off S, or unreached)."""
    g = np.where(K, np.int64(0), FAR)
    while True:
        nxt = np.where(S, np.minimum(g, _neighbour_min(g, conn, FAR) + 1), FAR)
        nxt = np.where(nxt >= FAR, FAR, nxt)
        if (nxt == g).all():
            return g
        g = nxt


def anchors(S, K, conn):
    """(a int64 [nz, ny, nx]: the anchor, n (the voxel count) off S; g; reached bool)."""
    n = S.size
    g = steps(S, K, conn)
    reached = S & (g < FAR)
    a = np.where(K, NL.first_of_component(K, conn), n).astype(np.int64)
    top = int(g[reached].max()) if reached.any() else 0
    for k in range(1, top + 1):
        closer = np.where(S & (g == k - 1), a, n)
        a = np.where(g == k, _neighbour_min(closer, conn, np.int64(n)), a)
    rest = S & ~reached
    a = np.where(rest, NL.first_of_component(rest, conn), a)
    return a, g, reached


def apply(vol, kind, lo, hi, conn, box, spacing, radius, fill_out):
    """(labels uint32, table uint64 [N, 8], result uint64 [8], dense, g uint32 with 0xffffffff where it is not finite)."""
    v = np.asarray(vol)
    S = NL.foreground(v, kind, lo, hi, box)
    K = S & ND.ero(S, spacing, ND.r2_of(radius))
    a, g, reached = anchors(S, K, conn)
    roots = np.unique(a[S])
    labels = np.zeros(S.shape, np.uint32)
    labels[S] = (np.searchsorted(roots, a[S]) + 1).astype(np.uint32)
    table = np.zeros((len(roots), 8), np.uint64)
    if len(roots):
        ids = labels[S].astype(np.int64) - 1
        z, y, x = (c[S] for c in np.indices(S.shape))
        table[:, 0] = np.bincount(ids, minlength=len(roots))
        table[:, 1] = roots
        for col, c in ((2, x), (3, y), (4, z)):
            lo_c = np.full(len(roots), np.iinfo(np.int64).max)
            hi_c = np.zeros(len(roots), np.int64)
            np.minimum.at(lo_c, ids, c)
            np.maximum.at(hi_c, ids, c)
            table[:, col], table[:, col + 3] = lo_c, hi_c + 1
    big = np.int64(1) << 40
    ids_or_big = np.where(S, labels.astype(np.int64), big)
    cut = S & (_neighbour_min(ids_or_big, conn, big) < labels.astype(np.int64))
    dense = np.where(cut, np.full(v.shape, NL.fill_bits(fill_out, kind), v.dtype), v)
    rest = S & ~reached
    is_anchor = np.zeros(S.size, bool)
    is_anchor[roots] = True
    is_anchor = is_anchor.reshape(S.shape)
    result = np.array([len(roots), int(S.sum()), int((is_anchor & K).sum()), int(K.sum()), int((is_anchor & rest).sum()), int(rest.sum()), int(cut.sum()),
                       int(g[reached].max()) if reached.any() else 0], np.uint64)
    return labels, table, result, dense, np.where(reached, g, 0xFFFFFFFF).astype(np.uint32)
