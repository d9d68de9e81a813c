"""vk_skeletonize in numpy, written another way than tests/skel_restatement.c: whole arrays and shifted views of a zero-padded set, the
26-bit neighbourhood mask of every voxel at once, and the simple-point test as a table over the masks that occur -- each entry decided
once by the reachability matrix of the mask's graph (Boolean matrix powers), not by a flood fill.  Nothing of the library is used."""
import numpy as np

import np_label_reference as NL

CURVE, KERNEL = 0, 1
# bit k of a mask: the neighbour at offset o = k (k < 13) or k + 1, d = (o % 3 - 1, o // 3 % 3 - 1, o // 9 - 1) as (dx, dy, dz)
OFFSETS = [(o % 3 - 1, o // 3 % 3 - 1, o // 9 - 1) for o in range(27) if o != 13]
_D = np.array(OFFSETS)
_ADJ26 = (np.abs(_D[:, None, :] - _D[None, :, :]).max(axis=2) == 1)
_L1 = np.abs(_D).sum(axis=1)
_EIGHTEEN = np.flatnonzero(_L1 <= 2)
_FACES = np.flatnonzero(_L1 == 1)
_ADJ6 = (np.abs(_D[:, None, :] - _D[None, :, :]).sum(axis=2) == 1)
_SIMPLE = {}


def _reach(adj, members):
    """The reachability matrix among `members` (indices) over adj: (I + A)^n by squaring."""
    a = adj[np.ix_(members, members)] | np.eye(len(members), dtype=bool)
    for _ in range(5):  # 2^5 >= 26
        a = (a.astype(np.uint8) @ a.astype(np.uint8)) > 0
    return a


def simple(m):
    """The header's skel_simple of one 26-bit mask."""
    m = int(m)
    if m not in _SIMPLE:
        bits = np.array([(m >> k) & 1 for k in range(26)], bool)
        on = np.flatnonzero(bits)
        ok = len(on) > 0 and bool(_reach(_ADJ26, on)[0].all())           # (a) one 26-component of set bits
        if ok:
            off = np.array([k for k in _EIGHTEEN if not bits[k]], int)
            faces = [j for j, k in enumerate(off) if k in _FACES]
            ok = len(faces) > 0
            if ok:
                r = _reach(_ADJ6, off)
                ok = bool(r[faces[0]][faces].all())                      # (b) every clear face in the first one's 6-component
        _SIMPLE[m] = ok
    return _SIMPLE[m]


def masks(k):
    """uint32 [nz, ny, nx]: every voxel's neighbourhood mask over the set k (bool), background outside the array."""
    nz, ny, nx = k.shape
    p = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    p[1:-1, 1:-1, 1:-1] = k
    m = np.zeros(k.shape, np.uint32)
    for b, (dx, dy, dz) in enumerate(OFFSETS):
        m |= p[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx].astype(np.uint32) << np.uint32(b)
    return m


def popcount(m):
    c = np.zeros(m.shape, np.uint32)
    for b in range(26):
        c += (m >> np.uint32(b)) & np.uint32(1)
    return c


def candidates(k):
    """The voxels of k with a face neighbour outside k."""
    m = masks(k)
    face_bits = np.uint32(sum(1 << int(b) for b in _FACES))
    return k & ((m & face_bits) != face_bits)


def thin(s, mode, max_iterations=0):
    """(K bool, iterations that deleted something, converged)."""
    k = s.copy()
    z, y, x = np.indices(k.shape)
    sf = (x & 1) | ((y & 1) << 1) | ((z & 1) << 2)
    iterations = 0
    while max_iterations == 0 or iterations < max_iterations:
        cand = candidates(k)
        deleted = 0
        for sub in range(8):
            m = masks(k)
            look = k & cand & (sf == sub)
            if mode == CURVE:
                look &= popcount(m) != 1
            if not look.any():
                continue
            occurring, where = np.unique(m[look], return_inverse=True)  # the table: one entry per mask that occurs
            table = np.array([simple(v) for v in occurring], bool)
            gone = np.zeros(k.shape, bool)
            gone[look] = table[where.ravel()]
            k &= ~gone
            deleted += int(gone.sum())
        if deleted == 0:
            return k, iterations, 1
        iterations += 1
    return k, iterations, 0


def classes_of(k):
    return np.where(k, np.minimum(popcount(masks(k)), 3) + 1, 0).astype(np.uint8)


def links_of(k):
    m = masks(k)
    return [int((k & (((m >> np.uint32(13 + j)) & np.uint32(1)) != 0)).sum()) for j in range(13)]


def apply(vol, kind, lo, hi, mode, max_iterations, fill_in, fill_out, box):
    """(classes uint8 [nz, ny, nx], dense, result uint64 [21]: n_foreground, n_skeleton, n_isolated, n_end, n_regular, n_junction,
    links[13], iterations, converged).  fill_in None: a voxel of K keeps its stored bits."""
    v = np.asarray(vol)
    s = NL.foreground(v, kind, lo, hi, box)
    k, iterations, converged = thin(s, mode, max_iterations)
    cls = classes_of(k)
    inside = v if fill_in is None else np.full(v.shape, NL.fill_bits(fill_in, kind), v.dtype)
    dense = np.where(k, inside, np.full(v.shape, NL.fill_bits(fill_out, kind), v.dtype)).astype(v.dtype)
    result = np.array([s.sum(), k.sum()] + [int((cls == c).sum()) for c in (1, 2, 3, 4)] + links_of(k) + [iterations, converged], np.uint64)
    return cls, dense, result
