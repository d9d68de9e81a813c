"""The shared cases of vk_skeletonize: volumes as small as can still break a tile, a halo, a subfield or an
iteration -- extents of 1, extents that are no multiple of the tile (32 x 16 x 8) and one that is, 3 x 3 x 3 tiles, shapes that straddle a
tile corner, boxes whose origin is odd -- each in u8, u16 and f16, with the requests that run on them.  Dimensions are (nx, ny, nz);
arrays are [nz, ny, nx]."""
import collections
import math

import numpy as np

import dist_cases as DC
import label_cases as LC

INF = math.inf
MAX_VOXELS = 64000
TILE = LC.TILE
CURVE, KERNEL = 0, 1
MODE_NAME = {CURVE: "curve", KERNEL: "kernel"}
DIMS = ((1, 1, 1), (70, 1, 1), (1, 70, 1), (1, 1, 70), (7, 9, 17), (33, 17, 9), (35, 19, 17), (64, 32, 16))
BIG = (70, 35, 18)      # 3 x 3 x 3 tiles
SHAPES = (48, 32, 18)   # 2 x 2 x 3 tiles; the shapes sit on the tile corner (32, 16, 8)
CORNER = (32, 16, 8)
LINE = (160, 1, 1)      # five tiles in a row
ODD_BOX = (5, 3, 1, 50, 31, 15)
ODD_CLIP = ((0.1, 0.09, 0.15), (0.9, 0.8, 1.0))

# fill_in: None keeps the stored bits on K, a number stores F(fill_in) there (VK_SKEL_FILL_IN).  box: None or (x0, y0, z0, x1, y1, z1);
# clip: None or (lo3, hi3) -- the box is then the clip box's voxel box and the call passes VK_SKEL_CLIP_BOX.
Case = collections.namedtuple("Case", "name vol_id vol kind lo hi mode max_iterations fill_in fill_out box clip")


def _grid(d):
    z, y, x = np.indices(LC.shape(d))
    return x, y, z


def bar(d=SHAPES):
    """5 x 5 in cross-section, 24 long along x, through the tile corner."""
    m = np.zeros(LC.shape(d), bool)
    m[6:11, 14:19, 20:44] = True
    return m


def plate(d=SHAPES):
    """3 thick along z, 20 x 20 across, over the tile corner."""
    m = np.zeros(LC.shape(d), bool)
    m[7:10, 6:26, 22:42] = True
    return m


def ball(d=SHAPES, r=6.5):
    """13 voxels thick: several iterations to thin."""
    x, y, z = _grid(d)
    return (x - CORNER[0]) ** 2 + (y - CORNER[1]) ** 2 + (z - CORNER[2]) ** 2 <= r * r


def shell(d=SHAPES):
    """A hollow ball: one cavity."""
    return ball(d, 7.2) & ~ball(d, 4.8)


def ring(d=SHAPES):
    """A solid torus around the z axis through the corner: one tunnel."""
    x, y, z = _grid(d)
    rho = np.sqrt((x - CORNER[0]) ** 2.0 + (y - CORNER[1]) ** 2.0)
    return (rho - 9.0) ** 2 + (z - CORNER[2]) ** 2 <= 2.3 ** 2


def tube_torus(d=SHAPES):
    """The wall of a torus-shaped tube: two tunnels and one cavity."""
    x, y, z = _grid(d)
    rho = np.sqrt((x - CORNER[0]) ** 2.0 + (y - CORNER[1]) ** 2.0)
    q = (rho - 9.0) ** 2 + (z - CORNER[2]) ** 2
    return (q <= 4.4 ** 2) & (q >= 2.4 ** 2)


def fixed_bar():
    """The first fixed case: a full (26, 5, 5) volume, the issue's 5 x 5 x 26 bar."""
    return np.ones(LC.shape((26, 5, 5)), bool)


def fixed_slabs():
    """The second fixed case: (12, 7, 3), everything but three slabs through every z and one voxel; |S| = 206."""
    m = np.ones(LC.shape((12, 7, 3)), bool)
    m[:, 0:6, 3] = False
    m[:, 1:7, 7] = False
    m[:, 2:5, 5] = False
    m[1, 3, 10] = False
    return m


def _make(kind, vol_id, vol, mode, lo=0.5, hi=INF, max_iterations=0, fill_in=None, fill_out=0.0, box=None, clip=None, tag=""):
    d = tuple(reversed(vol.shape))
    if clip is not None:
        box = LC.clip_voxel_box(clip[0], clip[1], d)
    where = ", box %s" % (box,) if box is not None and clip is None else (", clip box" if clip is not None else "")
    stop = f" at most {max_iterations} iterations" if max_iterations else ""
    name = f"{vol_id}, [{lo}, {hi}] {MODE_NAME[mode]}{stop} fill_in {fill_in} fill_out {fill_out}{where}{tag}"
    return Case(name, vol_id, vol, kind, float(lo), float(hi), mode, int(max_iterations), None if fill_in is None else float(fill_in), float(fill_out), box, clip)


_CACHE = []


def cases():
    if _CACHE:
        return _CACHE
    out = []
    for kind in ("u8", "u16", "f16"):
        # every dimension: random sets of rotating density, mode and fill
        for k, d in enumerate(DIMS):
            density = (0.35, 0.6, 0.85)[k % 3]
            out.append(_make(kind, f"{kind} {d} random at density {density}", LC.percolation(d, kind, 120 + k, density), mode=(CURVE, KERNEL)[k % 2], fill_in=(None, 1.0)[(k // 2) % 2],
                             fill_out=(0.0, 0.25)[k % 2]))
        # the elementary sets on an odd volume of 2 x 2 x 2 tiles
        d = (37, 21, 11)
        full = DC.mask_volume(np.ones(LC.shape(d), bool), kind)
        out.append(_make(kind, f"{kind} {d} empty", DC.mask_volume(np.zeros(LC.shape(d), bool), kind), mode=CURVE, fill_out=0.5))
        out.append(_make(kind, f"{kind} {d} full", full, mode=CURVE))
        out.append(_make(kind, f"{kind} {d} full", full, mode=KERNEL, fill_in=0.75))
        # the shapes on a tile corner
        for word, mask, mode in (("a bar", bar(), CURVE), ("a plate", plate(), CURVE), ("a plate", plate(), KERNEL), ("a ball", ball(), KERNEL), ("a ball", ball(), CURVE), ("a ring", ring(), KERNEL),
                                 ("a hollow shell", shell(), KERNEL), ("a tube-wall torus", tube_torus(), KERNEL), ("a tube-wall torus", tube_torus(), CURVE)):
            out.append(_make(kind, f"{kind} {SHAPES} {word} on the tile corner", DC.mask_volume(mask, kind), mode=mode))
        out.append(_make(kind, f"{kind} {SHAPES} a ball on the tile corner", DC.mask_volume(ball(), kind), mode=KERNEL, max_iterations=2, fill_in=1.0, tag=", stopped early"))
        # the fixed cases
        out.append(_make(kind, f"{kind} (26, 5, 5) the fixed bar", DC.mask_volume(fixed_bar(), kind), mode=CURVE))
        out.append(_make(kind, f"{kind} (12, 7, 3) the fixed slabs", DC.mask_volume(fixed_slabs(), kind), mode=KERNEL))
        # a line through five tiles: in kernel mode it shrinks from both ends, and the middle tile sleeps until an end comes near
        out.append(_make(kind, f"{kind} {LINE} a line through five tiles", DC.mask_volume(np.ones(LC.shape(LINE), bool), kind), mode=KERNEL))
        # random sets on 3 x 3 x 3 tiles
        for density, mode, fill_in in ((0.31, CURVE, None), (0.6, KERNEL, None), (0.9, CURVE, 0.5)):
            out.append(_make(kind, f"{kind} {BIG} percolation at density {density}", LC.percolation(BIG, kind, 11, density), mode=mode, fill_in=fill_in))
        vol, vid = LC.percolation(BIG, kind, 11, 0.9), f"{kind} {BIG} percolation at density 0.9"
        out.append(_make(kind, vid, vol, mode=KERNEL, box=ODD_BOX, fill_out=0.125))
        out.append(_make(kind, vid, vol, mode=CURVE, box=(7, 7, 7, 7, 9, 9), tag=", empty box"))
        out.append(_make(kind, vid, vol, mode=CURVE, clip=ODD_CLIP, fill_out=0.25))
        out.append(_make(kind, vid, vol, mode=CURVE, max_iterations=1, tag=", stopped early"))
        # graded data and a two-sided range
        vol, vid = LC.noise((25, 19, 21), kind, 77), f"{kind} (25, 19, 21) uniform noise"
        out.append(_make(kind, vid, vol, mode=CURVE, lo=0.2, hi=0.9))
        out.append(_make(kind, vid, vol, mode=KERNEL, lo=-INF, hi=0.8, fill_in=0.0, fill_out=1.0))
    # f16: NaN, infinities, zeros of both signs, denormals
    vol, vid = LC.f16_specials((37, 21, 11), 3), "f16 (37, 21, 11) NaN, inf, -0, denormals"
    for j, (lo, hi) in enumerate(((-INF, INF), (0.0, INF), (-INF, 0.0), (INF, INF), (-INF, -INF), (0.0, 0.0))):
        out.append(_make("f16", vid, vol, mode=(CURVE, KERNEL)[j % 2], lo=lo, hi=hi, fill_in=(None, -0.0)[j % 2], fill_out=-0.0 if j % 2 else 0.5))
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.vol.setflags(write=False)
        assert c.vol.size <= MAX_VOXELS
    _CACHE.extend(out)
    return _CACHE
