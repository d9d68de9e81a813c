"""vk_label_components restated in numpy from the rule in include/vokselis_hip.h: every foreground voxel starts with its own linear index,
takes the smallest label among its neighbours and itself, and follows labels to their labels, until nothing changes -- the label of a
voxel is then its component's smallest index, `first`.  Numbering, table, selection and mask follow the header's words in whole-array
operations.  Shares nothing with the library's union-find or with the C restatement's flood fill."""
import numpy as np

SCALE = {"u8": np.float32(255.0), "u16": np.float32(65535.0)}


def bound(v, kind):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(v) * SCALE[kind] if kind in SCALE else np.float32(v)


def box_mask(shape3, box):
    m = np.zeros(shape3, bool)
    if box is None:
        m[...] = True
    else:
        x0, y0, z0, x1, y1, z1 = box
        m[z0:z1, y0:y1, x0:x1] = True
    return m


def foreground(vol, kind, lo, hi, box):
    t = np.asarray(vol).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (t >= bound(lo, kind)) & (t <= bound(hi, kind)) & box_mask(t.shape, box)


def offsets(conn):
    most = {6: 1, 18: 2, 26: 3}[conn]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 1 <= abs(dx) + abs(dy) + abs(dz) <= most]


def _shifted(n, d):
    """(destination, source) slices of an axis of n for the neighbour at offset d: no wrap."""
    return (slice(0, n - 1), slice(1, n)) if d == 1 else ((slice(1, n), slice(0, n - 1)) if d == -1 else (slice(0, n), slice(0, n)))


def first_of_component(fg, conn):
    """[nz, ny, nx] int64: the smallest linear index of each foreground voxel's component; n (the voxel count) on background."""
    n = fg.size
    lab = np.where(fg, np.arange(n, dtype=np.int64).reshape(fg.shape), n)
    while True:
        m = lab.copy()
        for d in offsets(conn):
            (dz, sz), (dy, sy), (dx, sx) = (_shifted(fg.shape[a], d[a]) for a in range(3))
            m[dz, dy, dx] = np.minimum(m[dz, dy, dx], lab[sz, sy, sx])
        m = np.where(fg, m, n)
        flat = m.ravel()
        sel = np.flatnonzero(fg.ravel())
        while True:  # a label is the index of a voxel of the same component: take that voxel's label
            nxt = flat[flat[sel]]
            if (nxt == flat[sel]).all():
                break
            flat[sel] = nxt
        if (m == lab).all():
            return lab
        lab = m


def label(vol, kind, lo, hi, conn, box):
    """(labels uint32 [nz, ny, nx], table uint64 [n, 8]: n_voxels, first, x0, y0, z0, x1, y1, z1)."""
    fg = foreground(vol, kind, lo, hi, box)
    first = first_of_component(fg, conn)
    roots = np.unique(first[fg])                       # increasing first: the numbering
    labels = np.zeros(fg.shape, np.uint32)
    labels[fg] = (np.searchsorted(roots, first[fg]) + 1).astype(np.uint32)
    table = np.zeros((len(roots), 8), np.uint64)
    if len(roots):
        ids = labels[fg].astype(np.int64) - 1
        z, y, x = (c[fg] for c in np.indices(fg.shape))
        table[:, 0] = np.bincount(ids, minlength=len(roots))
        table[:, 1] = roots
        for col, c in ((2, x), (3, y), (4, z)):
            lo_c = np.full(len(roots), np.iinfo(np.int64).max)
            hi_c = np.zeros(len(roots), np.int64)
            np.minimum.at(lo_c, ids, c)
            np.maximum.at(hi_c, ids, c)
            table[:, col], table[:, col + 3] = lo_c, hi_c + 1
    return labels, table


def select(table, labels, keep, count, seeds):
    """bool [n + 1]: whether id is selected (index 0: background, never)."""
    n = len(table)
    sel = np.zeros(n + 1, bool)
    sizes = table[:, 0].astype(np.int64)
    if keep == "all":
        sel[1:] = True
    elif keep == "largest":
        order = np.lexsort((table[:, 1].astype(np.int64), -sizes))  # n_voxels descending, then first ascending
        sel[order[:min(count, n)] + 1] = True
    elif keep == "min_size":
        sel[1:] = sizes >= count
    elif keep == "seeds":
        for x, y, z in seeds:
            sel[labels[z, y, x]] = True
        sel[0] = False
    else:
        raise ValueError(keep)
    return sel


def fill_bits(fill, kind):
    f = np.float32(fill)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return f.astype(np.float16)
    return np.rint(np.minimum(np.maximum(f * SCALE[kind], np.float32(0.0)), SCALE[kind])).astype(np.uint8 if kind == "u8" else np.uint16)


def apply(vol, kind, lo, hi, conn, box, keep, count, seeds, invert, fill):
    """(labels, table, result uint64 [4], dense)."""
    labels, table = label(vol, kind, lo, hi, conn, box)
    sel = select(table, labels, keep, count, seeds)
    m = sel[labels]
    stays = ~m if invert else m
    v = np.asarray(vol)
    dense = np.where(stays, v, np.full(v.shape, fill_bits(fill, kind), v.dtype))
    result = np.array([len(table), int(table[:, 0].sum()), int(sel.sum()), int(table[sel[1:], 0].sum())], np.uint64)
    return labels, table, result, dense


def renumber_by_first(lab):
    """A labelling with arbitrary positive ids -> ids by increasing first voxel in raster order (scipy.ndimage.label's output is
    already in that order for its own scan; this makes it so by construction)."""
    flat = np.asarray(lab).ravel()
    ids, first = np.unique(flat, return_index=True)
    keep = ids != 0
    ids, first = ids[keep], first[keep]
    new = np.zeros(int(flat.max()) + 1 if flat.size else 1, np.uint32)
    new[ids[np.argsort(first)]] = np.arange(1, len(ids) + 1, dtype=np.uint32)
    return new[flat].reshape(np.asarray(lab).shape)
