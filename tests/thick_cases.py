"""The shared cases of vk_local_thickness: volumes as small as can still break a tile, a window or a list -- extents
of 1, extents that are no multiple of the tile (8), walks that cross tiles on every side -- each in u8, u16 and f16, with the requests
that run on them.  Dimensions are (nx, ny, nz); arrays are [nz, ny, nx]."""
import collections
import math

import numpy as np

import dist_cases as DC
import label_cases as LC

INF = math.inf
MAX_VOXELS = 48 * 40 * 33
TILE = 8
DIMS = ((1, 1, 1), (70, 1, 1), (1, 70, 1), (1, 1, 70), (7, 9, 17), (17, 33, 9), (33, 7, 9), (25, 19, 21))
SPACINGS = ((1, 1, 1), (2, 2, 5), (3, 1, 2), (64, 64, 64))

# box: None or (x0, y0, z0, x1, y1, z1); clip: None or (lo3, hi3) -- the box is then the clip box's voxel box and the call passes VK_THICK_CLIP_BOX.
# gain: 0.0 asks for the automatic gain.
Case = collections.namedtuple("Case", "name vol_id vol kind lo hi spacing max_radius gain fill_out box clip")


def balls(d, centres):
    """The union of the balls (cx, cy, cz, r2): the voxels with squared index distance <= r2 from a centre."""
    z, y, x = np.indices(LC.shape(d))
    m = np.zeros(LC.shape(d), bool)
    for cx, cy, cz, r2 in centres:
        m |= (x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r2
    return m


def plate(d, thick):
    m = np.zeros(LC.shape(d), bool)
    m[:, 6:6 + thick, :] = True
    return m


def wedge(d):
    """A wedge along x: its thickness along y grows from 1 to ny - 2, so that there are many distinct T2."""
    nx, ny, nz = d
    z, y, x = np.indices(LC.shape(d))
    return (y >= 1) & (y <= 1 + (x * (ny - 3)) // max(nx - 1, 1)) & (z >= 1) & (z < nz - 1)


def fixed_case(kind="u8"):
    """The issue's fixed case: 40 x 32 x 24, ball A centre (12, 16, 12) r^2 <= 81, ball B centre (27, 16, 12) r^2 <= 25."""
    d = (40, 32, 24)
    return d, balls(d, ((12, 16, 12, 81),)), balls(d, ((27, 16, 12, 25),))


def _make(kind, vol_id, vol, max_radius, lo=0.5, hi=INF, spacing=(1, 1, 1), gain=0.0, fill_out=0.0, box=None, clip=None, tag=""):
    d = tuple(reversed(vol.shape))
    if clip is not None:
        box = LC.clip_voxel_box(clip[0], clip[1], d)
    where = ", box %s" % (box,) if box is not None and clip is None else (", clip box" if clip is not None else "")
    name = f"{vol_id}, [{lo}, {hi}] cap {max_radius} spacing {spacing} gain {gain}{where}{tag}"
    return Case(name, vol_id, vol, kind, float(lo), float(hi), tuple(spacing), float(max_radius), float(gain), float(fill_out), box, clip)


_CACHE = []


def cases():
    if _CACHE:
        return _CACHE
    out = []
    for kind in ("u8", "u16", "f16"):
        # every dimension: the complement of sparse noise (a thick set with holes), a rotating spacing, the cap at 3 voxels of the smallest pitch
        for k, d in enumerate(DIMS):
            m = ~(np.random.default_rng(60 + k).random(LC.shape(d)) < 0.08)
            sp = SPACINGS[k % 4]
            out.append(_make(kind, f"{kind} {d} solid with 8 % holes", DC.mask_volume(m, kind), 3.0 * min(sp), spacing=sp, gain=(0.0, 0.25)[k % 2] / min(sp)))
        # the elementary sets on an odd volume of 5 x 3 x 2 tiles
        d = (37, 21, 11)
        corner = np.zeros(LC.shape(d), bool)
        corner[-1, -1, -1] = True
        sets = [("empty", np.zeros(LC.shape(d), bool)), ("full", np.ones(LC.shape(d), bool)), ("one voxel at the far corner", corner), ("a plate 2 thick", plate(d, 2)),
                ("a plate 5 thick", plate(d, 5)), ("a wedge", wedge(d)), ("porous block with a gap", DC.porous_block(d))]
        for j, (word, m) in enumerate(sets):
            vol, vid = DC.mask_volume(m, kind), f"{kind} {d} {word}"
            out.append(_make(kind, vid, vol, 16.0, spacing=SPACINGS[j % 3], gain=0.0, fill_out=(0.0, 0.125)[j % 2]))
            out.append(_make(kind, vid, vol, 2.0, gain=0.5))
        # the largest allowed reach on a small volume: every window is the whole volume
        vol, vid = DC.mask_volume(np.ones(LC.shape(d), bool), kind), f"{kind} {d} full"
        out.append(_make(kind, vid, vol, 32.0, gain=1.0 / 32.0))
        out.append(_make(kind, vid, vol, 2048.0, spacing=(64, 64, 64)))
        vol, vid = DC.mask_volume(wedge(d), kind), f"{kind} {d} a wedge"
        out.append(_make(kind, vid, vol, 32.0))
        out.append(_make(kind, vid, vol, 64.0 * 32.0, spacing=(64, 64, 64), gain=1.0 / 1024.0))
        out.append(_make(kind, vid, vol, 12.0, spacing=(2, 2, 5)))
        out.append(_make(kind, vid, vol, 7.0, spacing=(3, 1, 2), gain=0.1))
        # the largest volume, 6 x 5 x 5 tiles: walks cross tiles on every side.  Two overlapping balls with the cap below, at and above
        # the largest D (its largest D2 is 101: ball A's centre to the nearest voxel outside), a ball cut by the border, noise at two densities
        d = (48, 40, 33)
        two = balls(d, ((17, 20, 16, 100), (31, 18, 15, 49)))
        vol, vid = DC.mask_volume(two, kind), f"{kind} {d} two overlapping balls"
        for cap in (6.0, math.sqrt(101.0) + 1e-3, 10.04, 32.0):
            out.append(_make(kind, vid, vol, cap, gain=0.0 if cap != 6.0 else 0.15))
        out.append(_make(kind, vid, vol, 32.0, spacing=(2, 2, 5)))
        out.append(_make(kind, vid, vol, 32.0, spacing=(3, 1, 2), fill_out=0.5))
        out.append(_make(kind, vid, vol, 32.0 * 64.0, spacing=(64, 64, 64)))
        cut = balls(d, ((2, 20, 30, 144), (47, 0, 0, 81)))
        vol, vid = DC.mask_volume(cut, kind), f"{kind} {d} balls cut by the border"
        out.append(_make(kind, vid, vol, 32.0))
        out.append(_make(kind, vid, vol, 9.0, spacing=(1, 1, 1), gain=0.1))
        for density in (0.31, 0.9):
            vol, vid = LC.percolation(d, kind, 7, density), f"{kind} {d} percolation at density {density}"
            out.append(_make(kind, vid, vol, 16.0))
            out.append(_make(kind, vid, vol, 8.0, spacing=(2, 2, 5), gain=0.05))
        vol, vid = LC.percolation(d, kind, 7, 0.9), f"{kind} {d} percolation at density 0.9"
        out.append(_make(kind, vid, vol, 16.0, box=(5, 3, 2, 30, 31, 20)))
        out.append(_make(kind, vid, vol, 16.0, box=(7, 7, 7, 7, 9, 9), tag=", empty box"))
        out.append(_make(kind, vid, vol, 16.0, clip=((0.1, 0.0, 0.2), (0.9, 0.7, 1.0)), fill_out=0.25))
        # graded data and a two-sided range
        vol, vid = LC.noise((25, 19, 21), kind, 77), f"{kind} (25, 19, 21) uniform noise"
        out.append(_make(kind, vid, vol, 4.0, lo=0.2, hi=0.9, spacing=(2, 2, 5)))
        out.append(_make(kind, vid, vol, 4.0, lo=-INF, hi=0.8, gain=0.3, fill_out=1.0))
    # f16: NaN, infinities, zeros of both signs, denormals
    vol, vid = LC.f16_specials((37, 21, 11), 3), "f16 (37, 21, 11) NaN, inf, -0, denormals"
    for j, (lo, hi) in enumerate(((-INF, INF), (0.0, INF), (-INF, 0.0), (0.0, 0.0), (INF, INF), (-INF, -INF), (-1.0, 1.0))):
        out.append(_make("f16", vid, vol, 5.0, lo=lo, hi=hi, spacing=SPACINGS[j % 3], gain=(0.0, 3.0)[j % 2], fill_out=-0.0 if j % 2 else 0.5))
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.vol.setflags(write=False)
        assert c.vol.size <= MAX_VOXELS
    _CACHE.extend(out)
    return _CACHE
