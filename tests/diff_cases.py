"""The shared cases of vk_steady_diffusion: volumes as small as can still break a tile, a colour or a block --
extents of 1 on each axis (also along the axis of the flow, where a voxel lies on both faces), extents that are and are not multiples of
the tile (32 x 16 x 8), 3 x 3 x 3 tiles -- each in u8, u16 and f16, with the requests that run on them.  Most cases stop at 64 sweeps,
far from convergence: the equality with the references holds at any sweep count.  Dimensions are (nx, ny, nz); arrays are [nz, ny, nx]."""
import collections
import math

import numpy as np

import dist_cases as DC
import geo_cases as GC
import label_cases as LC

INF = math.inf
MAX_VOXELS = 64000
TILE = LC.TILE
DIMS = ((1, 1, 1), (70, 1, 1), (1, 70, 1), (1, 1, 70), (7, 9, 17), (33, 17, 9), (35, 19, 17), (64, 32, 16))
BIG = (70, 35, 18)   # 3 x 3 x 3 tiles
SPACINGS = ((1, 1, 1), (1, 1, 3), (2, 1, 1), (1, 2, 3))
OMEGAS = (0.0, 0.8, 1.0, 1.9)
CHECKS = (1, 4, 32)
CAP = 64
LONG = 20000

# omega: 0.0 asks for the automatic one.  box: None or (x0, y0, z0, x1, y1, z1); clip: None or (lo3, hi3) -- the box is then the clip
# box's voxel box and the call passes VK_DIFF_CLIP_BOX.  gain: 0.0 asks for 1.
Case = collections.namedtuple("Case", "name vol_id vol kind lo hi axis spacing omega check_every max_sweeps delta_tol flux_tol gain fill_out box clip")


def fixed_block():
    return np.ones(LC.shape((12, 7, 3)), bool)


def no_inlet(d):
    """Full, but for the whole first plane along x."""
    m = np.ones(LC.shape(d), bool)
    m[:, :, 0] = False
    return m


def sealed_pocket(d):
    """A full block with a closed shell of background around an interior block: the block inside touches neither face."""
    nx, ny, nz = d
    m = np.ones(LC.shape(d), bool)
    m[2:nz - 2, 3:ny - 3, 4:nx - 4] = False
    m[3:nz - 3, 4:ny - 4, 5:nx - 5] = True
    return m


def pocket_mask(d):
    nx, ny, nz = d
    m = np.zeros(LC.shape(d), bool)
    m[3:nz - 3, 4:ny - 4, 5:nx - 5] = True
    return m


def lone(d):
    """One voxel in the interior: den == 0."""
    nx, ny, nz = d
    m = np.zeros(LC.shape(d), bool)
    m[nz // 2, ny // 2, nx // 2] = True
    return m


def slabs(d):
    """Every second plane of constant y: straight channels along x and z, porosity 1 / 2 for an even ny."""
    m = np.zeros(LC.shape(d), bool)
    m[:, ::2, :] = True
    return m


def constriction(d):
    """Two chambers along x and a wall between them with one hole."""
    nx, ny, nz = d
    m = np.ones(LC.shape(d), bool)
    m[:, :, nx // 2] = False
    m[nz // 2, ny // 2, nx // 2] = True
    return m


def auto_omega(n_a):
    return float(np.float32(2.0 / (1.0 + 3.141592653589793 / float(n_a + 1))))


def extent(c):
    d = tuple(reversed(c.vol.shape))
    return d if c.box is None else (max(c.box[3] - c.box[0], 0), max(c.box[4] - c.box[1], 0), max(c.box[5] - c.box[2], 0))


def omega_used(c):
    """The omega a reference is given: the case's, or the automatic one of its box."""
    return float(np.float32(c.omega)) if c.omega != 0.0 else auto_omega(extent(c)[c.axis])


def _make(kind, vol_id, vol, axis=0, lo=0.5, hi=INF, spacing=(1, 1, 1), omega=0.0, check_every=32, max_sweeps=CAP, delta_tol=1e-5, flux_tol=1e-3, gain=0.0, fill_out=0.0, box=None,
          clip=None, tag=""):
    d = tuple(reversed(vol.shape))
    if clip is not None:
        box = LC.clip_voxel_box(clip[0], clip[1], d)
    where = ", box %s" % (box,) if box is not None and clip is None else (", clip box" if clip is not None else "")
    name = f"{vol_id}, [{lo}, {hi}] along {'xyz'[axis]} spacing {spacing} omega {omega} every {check_every} of {max_sweeps} tol {delta_tol} {flux_tol} gain {gain}{where}{tag}"
    return Case(name, vol_id, vol, kind, float(lo), float(hi), axis, tuple(spacing), float(omega), check_every, max_sweeps, float(delta_tol), float(flux_tol), float(gain), float(fill_out),
                box, clip)


_CACHE = []


def cases():
    if _CACHE:
        return _CACHE
    out = []
    for kind in ("u8", "u16", "f16"):
        # every dimension: the complement of sparse noise, a rotating axis, spacing, omega and block length
        for k, d in enumerate(DIMS):
            m = ~(np.random.default_rng(190 + k).random(LC.shape(d)) < 0.08)
            out.append(_make(kind, f"{kind} {d} solid with 8 % holes", DC.mask_volume(m, kind), axis=k % 3, spacing=SPACINGS[k % 4], omega=OMEGAS[k % 4], check_every=CHECKS[k % 3],
                             gain=(0.0, 0.5)[k % 2], fill_out=(0.0, 1.0)[k % 2]))
        # lines along the flow run to convergence: the longest cancellation in 1 - c
        line = DC.mask_volume(np.ones(LC.shape((70, 1, 1)), bool), kind)
        out.append(_make(kind, f"{kind} (70, 1, 1) a full line", line, axis=0, max_sweeps=LONG, tag=", to convergence"))
        # the elementary sets on an odd volume of 2 x 2 x 2 tiles
        d = (37, 21, 11)
        full = DC.mask_volume(np.ones(LC.shape(d), bool), kind)
        out.append(_make(kind, f"{kind} {d} empty", DC.mask_volume(np.zeros(LC.shape(d), bool), kind), axis=1, tag=", converges in its first block"))
        out.append(_make(kind, f"{kind} {d} full", full, axis=2, max_sweeps=LONG, tag=", to convergence"))
        out.append(_make(kind, f"{kind} {d} full", full, axis=0, spacing=(1, 2, 3), omega=1.9, check_every=4))
        out.append(_make(kind, f"{kind} {d} full", full, axis=1, spacing=(2, 1, 1), omega=0.8, check_every=1, max_sweeps=7, gain=2.0))
        out.append(_make(kind, f"{kind} {d} no voxel on the inlet", DC.mask_volume(no_inlet(d), kind), axis=0, check_every=4))
        out.append(_make(kind, f"{kind} {d} two blocks and a wall: nothing percolates", DC.mask_volume(GC.pocket(d), kind), axis=0, max_sweeps=LONG, tag=", to convergence"))
        out.append(_make(kind, f"{kind} {d} a sealed pocket", DC.mask_volume(sealed_pocket(d), kind), axis=0, max_sweeps=LONG, fill_out=0.25, tag=", to convergence"))
        out.append(_make(kind, f"{kind} (7, 9, 17) a lone voxel", DC.mask_volume(lone((7, 9, 17)), kind), axis=2, check_every=4, tag=", den == 0"))
        out.append(_make(kind, f"{kind} (12, 8, 5) parallel slabs", DC.mask_volume(slabs((12, 8, 5)), kind), axis=0, max_sweeps=LONG, tag=", to convergence"))
        out.append(_make(kind, f"{kind} (12, 8, 5) parallel slabs", DC.mask_volume(slabs((12, 8, 5)), kind), axis=2, spacing=(1, 1, 3), omega=1.0, check_every=4, max_sweeps=LONG,
                         tag=", to convergence"))
        out.append(_make(kind, f"{kind} (21, 9, 7) a constriction", DC.mask_volume(constriction((21, 9, 7)), kind), axis=0, max_sweeps=LONG, tag=", to convergence"))
        # the fixed cases
        out.append(_make(kind, f"{kind} (12, 7, 3) the full block", DC.mask_volume(fixed_block(), kind), axis=0, max_sweeps=LONG, tag=", to convergence"))
        out.append(_make(kind, f"{kind} (12, 7, 3) the fixed set", DC.mask_volume(GC.fixed_mask(), kind), axis=0, max_sweeps=LONG, tag=", to convergence"))
        for every in (4, 8, 16):  # the same solve in blocks of other lengths: convergence falls in other rounds of a batch
            out.append(_make(kind, f"{kind} (12, 7, 3) the fixed set", DC.mask_volume(GC.fixed_mask(), kind), axis=0, check_every=every, max_sweeps=LONG, tag=", to convergence"))
        # random sets on 3 x 3 x 3 tiles: near the 6-connected percolation threshold, and denser
        for density, axis, sp in ((0.31, 0, (1, 1, 1)), (0.6, 1, (1, 2, 3)), (0.9, 2, (2, 1, 1))):
            out.append(_make(kind, f"{kind} {BIG} random at density {density}", LC.percolation(BIG, kind, 11, density), axis=axis, spacing=sp))
        vol, vid = LC.percolation(BIG, kind, 11, 0.9), f"{kind} {BIG} random at density 0.9"
        out.append(_make(kind, vid, vol, axis=2, box=(5, 3, 2, 50, 31, 15), fill_out=0.125, omega=1.0))
        out.append(_make(kind, vid, vol, axis=0, box=(7, 7, 7, 7, 9, 9), tag=", empty box"))
        out.append(_make(kind, vid, vol, axis=1, spacing=(1, 1, 3), clip=((0.1, 0.0, 0.2), (0.9, 0.7, 1.0)), fill_out=0.25, gain=0.75, check_every=4))
        # graded data and a two-sided range
        vol, vid = LC.noise((25, 19, 21), kind, 77), f"{kind} (25, 19, 21) uniform noise"
        out.append(_make(kind, vid, vol, axis=2, lo=0.2, hi=0.9, spacing=(1, 2, 3)))
        out.append(_make(kind, vid, vol, axis=1, lo=-INF, hi=0.8, omega=1.9, check_every=1, max_sweeps=33, fill_out=1.0))
    # f16: NaN, infinities, zeros of both signs, denormals
    vol, vid = LC.f16_specials((37, 21, 11), 3), "f16 (37, 21, 11) NaN, inf, -0, denormals"
    for j, (lo, hi) in enumerate(((-INF, INF), (0.0, INF), (-INF, 0.0), (0.0, 0.0), (INF, INF), (-INF, -INF), (-1.0, 1.0))):
        out.append(_make("f16", vid, vol, axis=j % 3, lo=lo, hi=hi, spacing=SPACINGS[j % 4], omega=OMEGAS[j % 4], check_every=CHECKS[j % 3], fill_out=-0.0 if j % 2 else 0.5))
    assert len({c.name for c in out}) == len(out)
    assert 60 <= len(out) <= 150, len(out)
    for c in out:
        c.vol.setflags(write=False)
        assert c.vol.size <= MAX_VOXELS
    _CACHE.extend(out)
    return _CACHE
