"""The shared cases of vk_label_components: volumes as small as can still break a tile (32 x 16 x 8), a seam or the
numbering -- no dimension above 1 is a multiple of the tile's -- each in u8, u16 and f16, with the requests that run on them.  Dimensions
are (nx, ny, nz); arrays are [nz, ny, nx]."""
import collections
import math

import numpy as np

TILE = (32, 16, 8)
DTYPE = {"u8": np.uint8, "u16": np.uint16, "f16": np.float16}
TOP = {"u8": 255, "u16": 65535, "f16": 1.0}
INF = math.inf
MAX_VOXELS = 48 * 40 * 33

# box: None or (x0, y0, z0, x1, y1, z1); clip: None or (lo3, hi3) -- the box is then the clip box's voxel box and the call passes VK_LABEL_CLIP_BOX
Case = collections.namedtuple("Case", "name vol_id vol kind lo hi conn box clip keep count seeds invert fill")


def shape(d):
    return (d[2], d[1], d[0])


def clip_voxel_box(lo, hi, dims):
    """The voxels whose centre (i + 0.5) / n, in double, lies in [lo, hi] as f32: vk_volume_histogram's rule for the clip box."""
    out = []
    for a in range(3):
        l, h, n = float(np.float32(lo[a])), float(np.float32(hi[a])), dims[a]
        inside = [i for i in range(n) if l <= (i + 0.5) / n <= h]
        out.append((inside[0], inside[-1] + 1) if inside else (0, 0))
    return (out[0][0], out[1][0], out[2][0], out[0][1], out[1][1], out[2][1])


def _two_valued(mask, kind):
    return np.where(mask, DTYPE[kind](TOP[kind]), DTYPE[kind](0)).astype(DTYPE[kind])


def noise(d, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "f16":
        return rng.uniform(-1.0, 2.0, shape(d)).astype(np.float16)
    return rng.integers(0, TOP[kind] + 1, shape(d)).astype(DTYPE[kind])


def percolation(d, kind, seed, density=0.31):
    return _two_valued(np.random.default_rng(seed).random(shape(d)) < density, kind)


def checkerboard(d, kind):
    z, y, x = np.indices(shape(d))
    return _two_valued((x + y + z) % 2 == 0, kind)


def blocks(d, kind, touch):
    """Two blocks across the tile seams at x = 32, y = 16, z = 8 that touch only along an edge (they differ on two axes) or only at a
    corner (on three)."""
    m = np.zeros(shape(d), bool)
    m[5:8, 13:16, 28:32] = True
    if touch == "edge":
        m[5:8, 16:19, 32:35] = True
    else:
        m[8:10, 16:19, 32:35] = True
    return _two_valued(m, kind)


def serpentine(d, kind):
    """A one-voxel-wide path through every second row: along x, one voxel over to the next row, back along x; every second plane likewise."""
    nx, ny, nz = d
    m = np.zeros(shape(d), bool)
    flip = False
    for z in range(0, nz, 2):
        rows = list(range(0, ny, 2))
        if (z // 2) % 2:
            rows.reverse()
        for k, y in enumerate(rows):
            m[z, y, :] = True
            if k + 1 < len(rows):
                m[z, min(y, rows[k + 1]):max(y, rows[k + 1]) + 1, 0 if flip else nx - 1] = True
                flip = not flip
        if z + 2 < nz:
            m[z:z + 3, rows[-1], 0 if flip else nx - 1] = True
            flip = not flip
    return _two_valued(m, kind)


def spiral(d, kind):
    """A square spiral in every second plane, wound inwards on one plane and joined to the next at its centre or its rim."""
    nx, ny, nz = d
    m = np.zeros(shape(d), bool)
    for z in range(0, nz, 2):
        x0, y0, x1, y1 = 0, 0, nx - 1, ny - 1
        x, y = 0, 0
        m[z, y, x] = True
        while x1 - x0 >= 2 and y1 - y0 >= 2:
            m[z, y0, x0:x1 + 1] = True
            m[z, y0:y1 + 1, x1] = True
            m[z, y1, x0 + 2:x1 + 1] = True
            m[z, y0 + 2:y1 + 1, x0 + 2] = True
            x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
            m[z, y0, x0] = True
        if z + 2 < nz:
            m[z + 1, 0, 0] = True  # the rims are joined; the windings make the chains
    return _two_valued(m, kind)


def u_shape(d, kind):
    """Two arms from the first plane to the last that meet only in the last tile in raster order."""
    nx, ny, nz = d
    m = np.zeros(shape(d), bool)
    m[:, 1, 2] = True
    m[:, ny - 2, nx - 3] = True
    m[nz - 1, 1:ny - 1, 2] = True
    m[nz - 1, ny - 2, 2:nx - 2] = True
    return _two_valued(m, kind)


def f16_specials(d, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, shape(d)).astype(np.float16)
    bits = v.view(np.uint16)
    pick = rng.integers(0, 12, shape(d))
    for k, b in enumerate((0x7E00, 0xFE01, 0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x83FF)):  # NaN, -NaN, +inf, -inf, +0, -0, denormals
        bits[pick == k] = b
    return v


DIMS = ((1, 1, 1), (70, 1, 1), (1, 1, 70), (37, 21, 11), (48, 40, 33), (35, 10, 9), (33, 9, 10), (35, 19, 17), (70, 19, 18))


def _requests_full(d, vol_id):
    """Every keep mode with and without INVERT, the boxes, fills that clamp and tie: for the volumes with many components."""
    nx, ny, nz = d
    out = []
    for invert in (False, True):
        tag = ", INVERT" if invert else ""
        out += [("keep all" + tag, dict(keep="all", invert=invert, fill=0.25)),
                ("largest 1" + tag, dict(keep="largest", count=1, invert=invert, fill=0.5)),              # 127.5 and 32767.5: ties to even
                ("largest 3, ties in size" + tag, dict(keep="largest", count=3, invert=invert, fill=-1.0)),  # clamped low
                ("largest 10^9, above n" + tag, dict(keep="largest", count=10 ** 9, invert=invert, fill=7.0)),  # clamped high; f16: 7
                ("min size 1" + tag, dict(keep="min_size", count=1, invert=invert, fill=0.0)),
                ("min size 4" + tag, dict(keep="min_size", count=4, invert=invert, fill=1.0)),
                ("min size 10^7, above the largest" + tag, dict(keep="min_size", count=10 ** 7, invert=invert, fill=0.1)),
                ("seeds: background, two in one component, one outside the box" + tag,
                 dict(keep="seeds", seeds="auto", invert=invert, fill=0.0, box=(0, 0, 0, nx, ny, max(nz - 2, 0)))),
                ("one seed" + tag, dict(keep="seeds", seeds="one", invert=invert, fill=70000.0 if "f16" in vol_id else 0.9))]  # f16: overflows to +inf
    out += [("empty box", dict(box=(3, 2, 1, 3, 9, 5))), ("box one voxel thick", dict(box=(0, 0, min(3, nz - 1), nx, ny, min(3, nz - 1) + 1), conn=26)),
            ("box that cuts components in two", dict(box=(0, 0, 0, nx // 2, ny, nz), keep="largest", count=2)),
            ("clip box", dict(clip=((0.1, 0.0, 0.2), (0.9, 0.7, 1.0)), keep="min_size", count=2, conn=18))]
    return out


def _make(kind, vol_id, vol, name, lo, hi, conn=6, box=None, clip=None, keep="all", count=0, seeds=(), invert=False, fill=0.0):
    d = tuple(reversed(vol.shape))
    if clip is not None:
        box = clip_voxel_box(clip[0], clip[1], d)
    if isinstance(seeds, str):
        seeds = _auto_seeds(vol, kind, lo, hi, box, seeds)
    return Case(f"{vol_id}, [{lo}, {hi}] conn {conn}, {name}", vol_id, vol, kind, float(lo), float(hi), conn, box, clip, keep, count, tuple(seeds), invert, float(fill))


def _auto_seeds(vol, kind, lo, hi, box, how):
    """Seeds chosen from the data: the first foreground voxel and its successor in a run of two (two seeds in one component), the first
    background voxel, a foreground voxel outside the box."""
    import np_label_reference as NL

    d = tuple(reversed(vol.shape))
    fg = NL.foreground(vol, kind, lo, hi, None)
    flat = fg.ravel()
    pair = np.flatnonzero(flat[:-1] & flat[1:] & (np.arange(flat.size - 1) % d[0] != d[0] - 1))
    where = lambda i: (int(i) % d[0], int(i) // d[0] % d[1], int(i) // (d[0] * d[1]))
    if how == "one":
        return [where(np.flatnonzero(flat)[len(np.flatnonzero(flat)) // 2])] if flat.any() else [(0, 0, 0)]
    seeds = []
    if len(pair):
        seeds += [where(pair[0]), where(pair[0] + 1)]
    if (~flat).any():
        seeds.append(where(np.flatnonzero(~flat)[0]))
    if box is not None:
        outside = np.flatnonzero(flat & ~NL.box_mask(vol.shape, box).ravel())
        if len(outside):
            seeds.append(where(outside[-1]))
    return seeds or [(0, 0, 0)]


_CACHE = []


def cases():
    if _CACHE:
        return _CACHE
    out = []
    for kind in ("u8", "u16", "f16"):
        top = TOP[kind]
        # uniform noise at several levels, on the degenerate and the odd dimensions
        for d in ((1, 1, 1), (70, 1, 1), (1, 1, 70), (37, 21, 11)):
            vol, vid = noise(d, kind, 11 + sum(d)), f"{kind} {d} uniform noise"
            for lo, hi in ((0.5, INF), (0.3, 0.6), (0.8, INF), (-INF, 0.2)):
                for conn in ((6, 26) if d == (37, 21, 11) else (6,)):
                    out.append(_make(kind, vid, vol, "keep all", lo, hi, conn))
            if d == (37, 21, 11):
                for name, kw in _requests_full(d, vid):
                    out.append(_make(kind, vid, vol, name, 0.55, INF, **kw))
        # the percolation threshold of the cubic lattice: components of every size across many seams
        d = (48, 40, 33)
        vol, vid = percolation(d, kind, 6), f"{kind} {d} percolation at density 0.31"
        for conn in (6, 18, 26):
            out.append(_make(kind, vid, vol, "keep all", 0.5, INF, conn))
        for name, kw in _requests_full(d, vid):
            out.append(_make(kind, vid, vol, name, 1.0, 1.0, **kw))  # lo == hi
        # all foreground, all background
        d = (37, 21, 11)
        for word, value in (("all foreground", top), ("all background", 0)):
            vol, vid = np.full(shape(d), value, DTYPE[kind]), f"{kind} {d} constant, {word}"
            out.append(_make(kind, vid, vol, "largest 1", 0.5, INF, 6, keep="largest", count=1, fill=0.3))
            out.append(_make(kind, vid, vol, "seeds, INVERT", 0.5, INF, 26, keep="seeds", seeds=[(0, 0, 0), (36, 20, 10)], invert=True, fill=0.3))
        # structures that tell the connectivities apart, and the longest chains
        for vid, vol in ((f"{kind} (35, 10, 9) checkerboard", checkerboard((35, 10, 9), kind)), (f"{kind} (37, 21, 11) two blocks touching along an edge", blocks((37, 21, 11), kind, "edge")),
                         (f"{kind} (37, 21, 11) two blocks touching at a corner", blocks((37, 21, 11), kind, "corner")), (f"{kind} (33, 9, 10) serpentine", serpentine((33, 9, 10), kind)),
                         (f"{kind} (35, 19, 17) spiral", spiral((35, 19, 17), kind)), (f"{kind} (70, 19, 18) U joined in the last tile", u_shape((70, 19, 18), kind))):
            for conn in (6, 18, 26):
                out.append(_make(kind, vid, vol, "keep all", 1.0, 1.0, conn))
            out.append(_make(kind, vid, vol, "largest 1, INVERT", 0.5, INF, 6, keep="largest", count=1, invert=True, fill=0.5))
    # f16: NaN, infinities, zeros of both signs, denormals
    vol, vid = f16_specials((37, 21, 11), 3), "f16 (37, 21, 11) NaN, inf, -0, denormals"
    for lo, hi in ((-INF, INF), (0.0, INF), (-INF, 0.0), (0.0, 0.0), (INF, INF), (-INF, -INF), (5.96e-8, 6.1e-5), (-1.0, 1.0)):
        for conn in (6, 26):
            out.append(_make("f16", vid, vol, "largest 2", lo, hi, conn, keep="largest", count=2, fill=-0.0))
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.vol.setflags(write=False)
    _CACHE.extend(out)
    return _CACHE
