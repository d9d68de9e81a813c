"""The shared cases of vk_geodesic_distance: volumes as small as can still break a tile, a halo or a round --
extents of 1, extents that are no multiple of the tile (32 x 16 x 8) and one that is, 3 x 3 x 3 tiles, fronts that re-enter a tile --
each in u8, u16 and f16, with the requests that run on them.  Dimensions are (nx, ny, nz); arrays are [nz, ny, nx]."""
import collections
import math

import numpy as np

import dist_cases as DC
import label_cases as LC

INF = math.inf
MAX_VOXELS = 64000
TILE = LC.TILE
DIMS = ((1, 1, 1), (70, 1, 1), (1, 70, 1), (1, 1, 70), (7, 9, 17), (33, 17, 9), (35, 19, 17), (64, 32, 16))
BIG = (70, 35, 18)   # 3 x 3 x 3 tiles
SPACINGS = ((1, 1, 1), (1, 2, 3), (3, 1, 1), (64, 64, 64))
FACE = {"x-": 1, "x+": 2, "y-": 4, "y+": 8, "z-": 16, "z+": 32}
FACES = tuple(FACE)
OPPOSITE = {"x-": "x+", "x+": "x-", "y-": "y+", "y+": "y-", "z-": "z+", "z+": "z-"}

# sources, targets: face masks; seeds: voxels (x, y, z).  box: None or (x0, y0, z0, x1, y1, z1); clip: None or (lo3, hi3) -- the box is
# then the clip box's voxel box and the call passes VK_GEO_CLIP_BOX.  gain: 0.0 asks for the automatic gain.
Case = collections.namedtuple("Case", "name vol_id vol kind lo hi conn spacing sources targets seeds gain fill_out fill_unreached box clip")


def fixed_mask():
    """The issue's first fixed case: 12 x 7 x 3, everything but three slabs through every z and one voxel; |S| = 206."""
    m = np.ones(LC.shape((12, 7, 3)), bool)
    m[:, 0:6, 3] = False
    m[:, 1:7, 7] = False
    m[:, 2:5, 5] = False
    m[1, 3, 10] = False
    return m


def second_fixed_mask():
    m = np.ones(LC.shape((5, 1, 1)), bool)
    m[0, 0, 2] = False
    return m


def pocket(d):
    """Two blocks with a wall of background between them: what lies behind the wall is unreachable from x-."""
    nx, ny, nz = d
    m = np.ones(LC.shape(d), bool)
    m[:, :, nx // 2] = False
    return m


def island(d):
    """A block in the interior: it touches no face."""
    nx, ny, nz = d
    m = np.zeros(LC.shape(d), bool)
    m[2:nz - 2, 3:ny - 3, 4:nx - 4] = True
    return m


SERPENTINE = (40, 9, 3)


def detour():
    """(9, 7, 2): a wall at x = 4 in the plane z = 0 with its gap at y = 6, and a bridge over the wall at y = 0 through z = 1.  From the seed
    (3, 0, 0) the voxel (5, 0, 0) is 4 steps away over the bridge and 14 around the wall: at a z pitch of 8 the 14 steps are the shorter way."""
    d = (9, 7, 2)
    m = np.zeros(LC.shape(d), bool)
    m[0] = True
    m[0, 0:6, 4] = False
    m[1, 0, 3:6] = True
    return d, m, (3, 0, 0), (5, 0, 0)


def shortcut(blocked=False):
    """(64, 32, 1), 2 x 2 tiles.  From the seed (0, 0, 0) a corridor winds through tile (0, 0) -- row 0, then rows 2, 4, .. 12 over
    x = 2 .. 31 -- and leaves it at (32, 12) into a corridor x = 32 .. 40 of tile (1, 0): one tile crossing, about 220 steps.  A second
    route runs down the column x = 0 into tile (0, 1), along the row y = 17 into tile (1, 1) and up the column x = 33 into the same
    corridor: three crossings, 55 steps.  blocked: the second route is cut."""
    d = (64, 32, 1)
    m = np.zeros(LC.shape(d), bool)
    p = m[0]
    p[0, 0:32] = True
    right = True
    for y in range(2, 13, 2):
        p[y, 2:32] = True
        p[y - 2:y + 1, 31 if right else 2] = True
        right = not right
    p[12, 32:41] = True
    p[0:18, 0] = True
    p[17, 0:34] = True
    p[13:18, 33] = True
    if blocked:
        p[17, 20] = False
    return d, m, (0, 0, 0), (36, 12, 0)


def _make(kind, vol_id, vol, conn=26, lo=0.5, hi=INF, spacing=(1, 1, 1), sources=("x-",), targets=("x+",), seeds=(), gain=0.0, fill_out=0.0, fill_unreached=0.0, box=None, clip=None, tag=""):
    d = tuple(reversed(vol.shape))
    if clip is not None:
        box = LC.clip_voxel_box(clip[0], clip[1], d)
    where = ", box %s" % (box,) if box is not None and clip is None else (", clip box" if clip is not None else "")
    name = f"{vol_id}, [{lo}, {hi}] conn {conn} spacing {spacing} from {'+'.join(sources) or 'no face'} seeds {tuple(seeds)} to {'+'.join(targets) or 'no face'} gain {gain}{where}{tag}"
    return Case(name, vol_id, vol, kind, float(lo), float(hi), conn, tuple(spacing), sum(FACE[f] for f in sources), sum(FACE[f] for f in targets), tuple(tuple(s) for s in seeds),
                float(gain), float(fill_out), float(fill_unreached), box, clip)


_CACHE = []


def cases():
    if _CACHE:
        return _CACHE
    out = []
    for kind in ("u8", "u16", "f16"):
        # every dimension: the complement of sparse noise, a rotating connectivity, spacing, source face (its opposite is the target) and gain
        for k, d in enumerate(DIMS):
            m = ~(np.random.default_rng(90 + k).random(LC.shape(d)) < 0.08)
            face = FACES[k % 6]
            out.append(_make(kind, f"{kind} {d} solid with 8 % holes", DC.mask_volume(m, kind), conn=(6, 18, 26)[k % 3], spacing=SPACINGS[k % 4], sources=(face,), targets=(OPPOSITE[face],),
                             gain=(0.0, 1.0 / 8192.0)[k % 2], fill_unreached=(0.0, 1.0)[k % 2]))
        # the elementary sets on an odd volume of 2 x 2 x 2 tiles
        d = (37, 21, 11)
        full = DC.mask_volume(np.ones(LC.shape(d), bool), kind)
        out.append(_make(kind, f"{kind} {d} empty", DC.mask_volume(np.zeros(LC.shape(d), bool), kind), conn=6))
        out.append(_make(kind, f"{kind} {d} full", full, conn=26, sources=("z+",), targets=("z-",)))
        out.append(_make(kind, f"{kind} {d} full", full, conn=18, spacing=(64, 64, 64), sources=("y-", "x+"), targets=("y+", "z-")))
        out.append(_make(kind, f"{kind} {d} full", full, conn=6, spacing=(3, 1, 1), sources=(), seeds=((36, 20, 10), (0, 0, 0), (17, 3, 9)), targets=("y+",), tag=", seeds alone"))
        out.append(_make(kind, f"{kind} {d} an island that touches no face", DC.mask_volume(island(d), kind), conn=26, tag=", no source on the set"))
        out.append(_make(kind, f"{kind} {d} an island that touches no face", DC.mask_volume(island(d), kind), conn=18, spacing=(1, 2, 3), sources=("y-",), seeds=((20, 10, 5), (0, 0, 0)),
                         targets=(), gain=1.0 / 16384.0, fill_out=0.25, tag=", a seed on the set and a seed off it"))
        out.append(_make(kind, f"{kind} {d} two blocks and a wall: an unreachable pocket", DC.mask_volume(pocket(d), kind), conn=26, spacing=(1, 2, 3), fill_unreached=1.0, fill_out=0.5))
        out.append(_make(kind, f"{kind} {d} two blocks and a wall: an unreachable pocket", DC.mask_volume(pocket(d), kind), conn=6, sources=("x-",), seeds=((30, 4, 4),), targets=("x+", "x-"),
                         tag=", a seed plus a face"))
        # the fixed cases
        out.append(_make(kind, f"{kind} (12, 7, 3) the fixed set", DC.mask_volume(fixed_mask(), kind), conn=26))
        out.append(_make(kind, f"{kind} (5, 1, 1) the second fixed set", DC.mask_volume(second_fixed_mask(), kind), conn=6))
        # a corridor one voxel wide that crosses the tile seam at x = 32 on every row
        vol, vid = LC.serpentine(SERPENTINE, kind), f"{kind} {SERPENTINE} serpentine"
        out.append(_make(kind, vid, vol, conn=6, sources=(), seeds=((0, 0, 0),), targets=("z+",)))
        out.append(_make(kind, vid, vol, conn=26, spacing=(1, 2, 3), sources=(), seeds=((0, 0, 0),), targets=("z+",), gain=1.0 / 65536.0))
        # a cheap detour: more steps, less length
        d, m, seed, _ = detour()
        out.append(_make(kind, f"{kind} {d} a wall, its gap and a bridge: the cheap detour", DC.mask_volume(m, kind), conn=6, spacing=(1, 1, 8), sources=(), seeds=(seed,), targets=("x+",)))
        out.append(_make(kind, f"{kind} {d} a wall, its gap and a bridge: the cheap detour", DC.mask_volume(m, kind), conn=26, spacing=(1, 1, 16), sources=(), seeds=(seed,), targets=("x+",)))
        # a late shortcut: the route with fewer tile crossings is the longer one
        d, m, seed, _ = shortcut()
        for conn in (6, 26) if kind == "u8" else (6,):
            out.append(_make(kind, f"{kind} {d} two routes: the late shortcut", DC.mask_volume(m, kind), conn=conn, sources=(), seeds=(seed,), targets=("x+",)))
        # random sets on 3 x 3 x 3 tiles: near the 6-connected percolation threshold, and denser
        for density, conn, sp in ((0.31, 6, (1, 1, 1)), (0.6, 18, (1, 2, 3)), (0.9, 26, (3, 1, 1))):
            out.append(_make(kind, f"{kind} {BIG} percolation at density {density}", LC.percolation(BIG, kind, 11, density), conn=conn, spacing=sp))
        vol, vid = LC.percolation(BIG, kind, 11, 0.9), f"{kind} {BIG} percolation at density 0.9"
        out.append(_make(kind, vid, vol, conn=6, sources=("z-",), targets=("z+",), box=(5, 3, 2, 50, 31, 15), fill_out=0.125))
        out.append(_make(kind, vid, vol, conn=26, box=(7, 7, 7, 7, 9, 9), tag=", empty box"))
        out.append(_make(kind, vid, vol, conn=18, spacing=(64, 64, 64), sources=("y+",), targets=("y-",), clip=((0.1, 0.0, 0.2), (0.9, 0.7, 1.0)), fill_out=0.25, gain=1.0 / (1 << 21)))
        # graded data and a two-sided range
        vol, vid = LC.noise((25, 19, 21), kind, 77), f"{kind} (25, 19, 21) uniform noise"
        out.append(_make(kind, vid, vol, conn=26, lo=0.2, hi=0.9, spacing=(1, 2, 3), sources=("z-",), targets=("z+",)))
        out.append(_make(kind, vid, vol, conn=18, lo=-INF, hi=0.8, sources=("y-", "y+"), targets=("x-",), gain=1.0 / 4096.0, fill_out=1.0, fill_unreached=0.5))
    # f16: NaN, infinities, zeros of both signs, denormals
    vol, vid = LC.f16_specials((37, 21, 11), 3), "f16 (37, 21, 11) NaN, inf, -0, denormals"
    for j, (lo, hi) in enumerate(((-INF, INF), (0.0, INF), (-INF, 0.0), (0.0, 0.0), (INF, INF), (-INF, -INF), (-1.0, 1.0))):
        out.append(_make("f16", vid, vol, conn=(6, 18, 26)[j % 3], lo=lo, hi=hi, spacing=SPACINGS[j % 4], sources=(FACES[j % 6],), targets=(OPPOSITE[FACES[j % 6]],), gain=(0.0, 1.0 / 2048.0)[j % 2],
                         fill_out=-0.0 if j % 2 else 0.5, fill_unreached=0.75))
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.vol.setflags(write=False)
        assert c.vol.size <= MAX_VOXELS
    _CACHE.extend(out)
    return _CACHE
