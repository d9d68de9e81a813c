"""The shared cases of vk_split_components: volumes as small as can still break a tile (32 x 16 x 8), a seam, a round
of the growth or the numbering -- no dimension above 1 is a multiple of the tile's -- with the requests that run on them.  Dimensions are
(nx, ny, nz); arrays are [nz, ny, nx].  The volume builders are label_cases'."""
import collections
import math

import numpy as np

import label_cases as LC

TILE = LC.TILE
INF = math.inf
MAX_VOXELS = 70 * 35 * 19
FIXED_DIMS = (37, 23, 21)

# box: None or (x0, y0, z0, x1, y1, z1); clip: None or (lo3, hi3) -- the box is then the clip box's voxel box and the call passes VK_SPLIT_CLIP_BOX
Case = collections.namedtuple("Case", "name vol_id vol kind lo hi conn box clip spacing radius fill_out")


def balls(d, centres, r2=64):
    z, y, x = np.indices(LC.shape(d))
    m = np.zeros(LC.shape(d), bool)
    for cx, cy, cz in centres:
        m |= (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r2
    return m


def fixed_mask():
    """Two balls of radius 8 that overlap, a wire out of the second and a ball of radius 1 on its own: 4049 voxels."""
    m = balls(FIXED_DIMS, ((10, 11, 10), (22, 11, 10)))
    m[10, 11, 30:36] = True
    m |= balls(FIXED_DIMS, ((34, 3, 3),), 1)
    return m


def blob_field(d, seed, count, r_lo, r_hi):
    """Overlapping balls of several radii: touching grains."""
    rng = np.random.default_rng(seed)
    m = np.zeros(LC.shape(d), bool)
    for _ in range(count):
        c = [int(rng.integers(0, n)) for n in d]
        r = float(rng.uniform(r_lo, r_hi))
        m |= balls(d, (c,), r * r)
    return m


def serpentine_with_blob(d, kind):
    """label_cases' serpentine with a 5 x 5 x 5 block over its first corner: one marker, and a path hundreds of voxels long to grow along."""
    m = LC.serpentine(d, kind) != 0
    m[0:5, 0:5, 0:5] = True
    return LC._two_valued(m, kind)


def dumbbell(kind):
    """Two 7 x 7 x 7 blocks joined by a bar of 21 voxels: the bar's middle voxel is as far from one block's marker as from the other's."""
    m = np.zeros(LC.shape((37, 9, 9)), bool)
    m[1:8, 1:8, 1:8] = True
    m[1:8, 1:8, 29:36] = True
    m[4, 4, 8:29] = True
    return LC._two_valued(m, kind)


def _make(kind, vol_id, vol, name, lo, hi, radius, conn=6, box=None, clip=None, spacing=(1, 1, 1), fill_out=0.0):
    d = tuple(reversed(vol.shape))
    if clip is not None:
        box = LC.clip_voxel_box(clip[0], clip[1], d)
    return Case(f"{vol_id}, [{lo}, {hi}] conn {conn} radius {radius}, {name}", vol_id, vol, kind, float(lo), float(hi), conn, box, clip, tuple(spacing), float(radius), float(fill_out))


_CACHE = []


def cases():
    if _CACHE:
        return _CACHE
    out = []
    # the fixed case
    vol, vid = LC._two_valued(fixed_mask(), "u8"), "u8 (37, 23, 21) two balls, a wire and a speck"
    for radius in (0.0, 3.0, 6.0, 7.5):
        out.append(_make("u8", vid, vol, "fixed", 0.5, INF, radius))
    # touching grains on the largest volume: more than two tiles on every axis
    d = (70, 35, 19)
    for kind, seed in (("u8", 4), ("u16", 5), ("f16", 6)):
        vol, vid = LC._two_valued(blob_field(d, seed, 14, 3.0, 7.0), kind), f"{kind} {d} overlapping balls"
        for conn, radius in ((6, 3.0), (18, 2.0), (26, 4.0)):
            out.append(_make(kind, vid, vol, "grains", 0.5, INF, radius, conn))
        out.append(_make(kind, vid, vol, "a box", 0.5, INF, 2.0, 6, box=(3, 2, 1, 60, 30, 17)))
        out.append(_make(kind, vid, vol, "the clip box", 0.5, INF, 2.0, 18, clip=((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))))
        out.append(_make(kind, vid, vol, "spacing (1, 1, 2)", 0.5, INF, 3.0, 6, spacing=(1, 1, 2), fill_out=0.25))
        out.append(_make(kind, vid, vol, "an empty box", 0.5, INF, 2.0, 6, box=(3, 2, 1, 3, 9, 5)))
    # a long growth: rounds >= 100
    for kind in ("u8", "u16"):
        out.append(_make(kind, f"{kind} (33, 9, 10) serpentine with a block", serpentine_with_blob((33, 9, 10), kind), "a long path", 1.0, 1.0, 2.0))
    # a tie between two anchors at equal g
    for kind, conn in (("u8", 6), ("f16", 26)):
        out.append(_make(kind, f"{kind} (37, 9, 9) dumbbell", dumbbell(kind), "a tie", 0.5, INF, 2.0, conn))
    # K empty, S empty, S the whole volume
    for kind in ("u8", "f16"):
        top = LC.TOP[kind]
        out.append(_make(kind, f"{kind} (35, 19, 17) percolation at density 0.31", LC.percolation((35, 19, 17), kind, 6), "K empty", 0.5, INF, 3.0))
        out.append(_make(kind, f"{kind} (37, 21, 11) constant, all background", np.full(LC.shape((37, 21, 11)), 0, LC.DTYPE[kind]), "S empty", 0.5, INF, 2.0))
        out.append(_make(kind, f"{kind} (37, 21, 11) constant, all foreground", np.full(LC.shape((37, 21, 11)), top, LC.DTYPE[kind]), "S whole", 0.5, INF, 5.0, 26))
    # a percolation field at radius 1: many small markers, residue beside them
    for kind, conn in (("u8", 6), ("u16", 18), ("f16", 26)):
        out.append(_make(kind, f"{kind} (35, 19, 17) percolation at density 0.62", LC.percolation((35, 19, 17), kind, 9, 0.62), "percolation", 0.5, INF, 1.0, conn))
    # a dimension of 1
    line = np.zeros(LC.shape((70, 1, 1)), bool)
    line[0, 0, 2:30] = True
    line[0, 0, 33:36] = True
    line[0, 0, 40:69] = True
    out.append(_make("u8", "u8 (70, 1, 1) three runs", LC._two_valued(line, "u8"), "a line", 0.5, INF, 2.0))
    out.append(_make("u16", "u16 (1, 1, 70) three runs", LC._two_valued(line.reshape(70, 1, 1), "u16"), "a column", 0.5, INF, 2.0, 26))
    plate = balls((37, 21, 1), ((9, 10, 0), (24, 10, 0)), 64)
    out.append(_make("u8", "u8 (37, 21, 1) two discs", LC._two_valued(plate, "u8"), "a plate", 0.5, INF, 5.0, 18))
    # f16: NaN, infinities, zeros of both signs, denormals
    vol, vid = LC.f16_specials((37, 21, 11), 3), "f16 (37, 21, 11) NaN, inf, -0, denormals"
    for lo, hi, radius, fill in ((-1.0, INF, 1.0, -2.0), (0.0, INF, 1.0, -1.0), (-INF, -0.0, 0.0, 1.0)):  # the fill lies outside the range
        for conn in (6, 26):
            out.append(_make("f16", vid, vol, "specials", lo, hi, radius, conn, fill_out=fill))
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.vol.setflags(write=False)
    _CACHE.extend(out)
    return _CACHE
