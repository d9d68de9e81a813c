"""The shared cases of vk_distance_transform: volumes as small as can still break a sweep, a line or a grid -- lines
longer than a wave (64) and than a workgroup (256) on every axis, no dimension above 3 a multiple of the wave or of the transpose's tile
(32) -- each in u8, u16 and f16,
with the requests that run on them.  Dimensions are (nx, ny, nz); arrays are [nz, ny, nx]."""
import collections
import math

import numpy as np

import label_cases as LC

INF = math.inf
MAX_VOXELS = 48 * 40 * 33
WAVE, WORKGROUP, TILE = 64, 256, 32   # the transposes of the x pass move tiles of 32 x 32
DIMS = ((1, 1, 1), (70, 1, 1), (1, 70, 1), (1, 1, 70), (300, 3, 2), (2, 300, 3), (3, 2, 300), (37, 21, 11), (48, 40, 33))
LONG = ((900, 1, 1), (1, 900, 1), (1, 1, 900))   # at spacing 64 the bound (64 * 899)^2 lies between 2^31 and 0xFFFFFFFE
REFUSED = (1100, 1, 1)                            # ... and (64 * 1099)^2 above it
SPACINGS = ((1, 1, 1), (2, 2, 5), (3, 1, 2), (64, 64, 64))
RADII = (0.0, 1.0, 1.5, 2.0, 3.3, 1000.0)
MORPH = ("dilate", "erode", "close", "open")

# box: None or (x0, y0, z0, x1, y1, z1); clip: None or (lo3, hi3) -- the box is then the clip box's voxel box and the call passes VK_DIST_CLIP_BOX
Case = collections.namedtuple("Case", "name vol_id vol kind lo hi op spacing radius fill_in fill_out box clip refused")


def mask_volume(mask, kind):
    return LC._two_valued(mask, kind)


def corner_masks(d):
    nx, ny, nz = d
    for k in range(8):
        m = np.zeros(LC.shape(d), bool)
        m[(nz - 1) * (k >> 2 & 1), (ny - 1) * (k >> 1 & 1), (nx - 1) * (k & 1)] = True
        yield k, m


def porous_block(d):
    """A solid block with one-voxel pores and a one-voxel gap that cuts it in two."""
    nx, ny, nz = d
    m = np.zeros(LC.shape(d), bool)
    m[2:nz - 2, 3:ny - 3, 4:nx - 4] = True
    rng = np.random.default_rng(5)
    for _ in range(12):  # pores: isolated single voxels well inside
        z, y, x = int(rng.integers(4, nz - 4)), int(rng.integers(5, ny - 5)), int(rng.integers(6, nx - 6))
        if m[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2].all():
            m[z, y, x] = False
    m[:, :, nx // 2] = False  # the gap: a plane one voxel thick
    return m


def bridged_blobs(d):
    """Two blobs joined by a bridge two voxels wide."""
    nx, ny, nz = d
    z, y, x = np.indices(LC.shape(d))
    cy, cz = ny // 2, nz // 2
    m = ((x - 9) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= 16) | ((x - (nx - 10)) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= 16)
    m[cz:cz + 2, cy:cy + 2, 9:nx - 9] = True
    return m


def _make(kind, vol_id, vol, op, lo=0.5, hi=INF, spacing=(1, 1, 1), radius=0.0, fill_in=1.0, fill_out=0.0, box=None, clip=None, refused=False, tag=""):
    d = tuple(reversed(vol.shape))
    if clip is not None:
        box = LC.clip_voxel_box(clip[0], clip[1], d)
    where = ", box %s" % (box,) if box is not None and clip is None else (", clip box" if clip is not None else "")
    name = f"{vol_id}, [{lo}, {hi}] {op} r {radius} spacing {spacing}{where}{tag}"
    return Case(name, vol_id, vol, kind, float(lo), float(hi), op, tuple(spacing), float(radius), float(fill_in), float(fill_out), box, clip, refused)


_CACHE = []


def cases():
    if _CACHE:
        return _CACHE
    out = []
    for kind in ("u8", "u16", "f16"):
        # every dimension: noise at the percolation density, both distances and a rotating morphology op, spacing and radius
        for k, d in enumerate(DIMS + LONG):
            vol, vid = LC.percolation(d, kind, 40 + k), f"{kind} {d} speckle at density 0.31"
            sp = SPACINGS[k % 3] if d not in LONG else SPACINGS[3]
            out.append(_make(kind, vid, vol, "outside", spacing=(1, 1, 1) if d not in LONG else sp))
            out.append(_make(kind, vid, vol, "inside", spacing=sp))
            out.append(_make(kind, vid, vol, MORPH[k % 4], spacing=sp, radius=RADII[1 + k % 4] * max(sp), fill_in=0.75, fill_out=0.25))
            if d in LONG:  # one voxel at the far end: the largest distance the bound allows
                far = np.zeros(LC.shape(d), bool)
                far[-1, -1, -1] = True
                out.append(_make(kind, f"{kind} {d} one voxel at the far corner", mask_volume(far, kind), "outside", spacing=sp))
        # the elementary sets on an odd volume
        d = (37, 21, 11)
        nx, ny, nz = d
        sets = [("empty", np.zeros(LC.shape(d), bool)), ("full", np.ones(LC.shape(d), bool))]
        sets += [(f"one voxel at corner {k}", m) for k, m in corner_masks(d)]
        mid = np.zeros(LC.shape(d), bool)
        mid[nz // 2, ny // 2, nx // 2] = True
        two = np.zeros(LC.shape(d), bool)
        two[0, 0, 0] = two[-1, -1, -1] = True
        plane = np.zeros(LC.shape(d), bool)
        plane[:, 8, :] = True
        sets += [("one voxel in the middle", mid), ("two voxels at opposite corners", two), ("a plane", plane)]
        for j, (word, m) in enumerate(sets):
            vol, vid = mask_volume(m, kind), f"{kind} {d} {word}"
            out.append(_make(kind, vid, vol, "outside", spacing=SPACINGS[j % 4]))
            out.append(_make(kind, vid, vol, "inside", spacing=SPACINGS[(j + 1) % 4]))
            if "corner" in word and word != "one voxel at corner 0" and "opposite" not in word:
                continue
            for op, r in zip(MORPH, (3.3, 1.0, 2.0, 1.5)):
                out.append(_make(kind, vid, vol, op, radius=r, fill_in=0.5, fill_out=0.125))
            out.append(_make(kind, vid, vol, "dilate", radius=1000.0))   # a radius larger than the volume
            out.append(_make(kind, vid, vol, "erode", radius=1000.0))
        # percolation at three densities on the largest volume: every op, every spacing, every radius
        d = (48, 40, 33)
        for density in (0.05, 0.31, 0.7):
            vol, vid = LC.percolation(d, kind, 7, density), f"{kind} {d} percolation at density {density}"
            for sp in SPACINGS:
                out.append(_make(kind, vid, vol, "outside", spacing=sp))
            out.append(_make(kind, vid, vol, "inside", spacing=(2, 2, 5)))
            for j, op in enumerate(MORPH):
                out.append(_make(kind, vid, vol, op, radius=RADII[1 + (j + int(density * 100)) % 5], spacing=(1, 1, 1), fill_in=0.9, fill_out=0.1))
            out.append(_make(kind, vid, vol, "close", radius=3.3 * 2, spacing=(2, 2, 5), fill_in=2.0, fill_out=-1.0))  # fills that clamp
            out.append(_make(kind, vid, vol, "open", radius=64.0 * 1.5, spacing=(64, 64, 64)))
        vol, vid = LC.percolation(d, kind, 7, 0.31), f"{kind} {d} percolation at density 0.31"
        out.append(_make(kind, vid, vol, "outside", box=(5, 3, 2, 30, 31, 20)))
        out.append(_make(kind, vid, vol, "inside", box=(5, 3, 2, 30, 31, 20), spacing=(3, 1, 2)))
        out.append(_make(kind, vid, vol, "close", radius=1.5, box=(5, 3, 2, 30, 31, 20), fill_in=0.5))
        out.append(_make(kind, vid, vol, "outside", box=(7, 7, 7, 7, 9, 9), tag=", empty box"))
        out.append(_make(kind, vid, vol, "outside", clip=((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))))
        out.append(_make(kind, vid, vol, "open", radius=1.0, clip=((0.1, 0.0, 0.2), (0.9, 0.7, 1.0)), fill_out=0.25))
        # radius 0 returns S under all four ops; close fills pores and a gap; open cuts a bridge
        d = (37, 21, 11)
        for word, m in (("porous block with a gap", porous_block(d)), ("two blobs joined by a bridge", bridged_blobs(d))):
            vol, vid = mask_volume(m, kind), f"{kind} {d} {word}"
            for op in MORPH:
                out.append(_make(kind, vid, vol, op, radius=0.0))
                out.append(_make(kind, vid, vol, op, radius=1.5, fill_in=1.0, fill_out=0.0))
            out.append(_make(kind, vid, vol, "outside"))
        # graded data and a two-sided range
        vol, vid = LC.noise((37, 21, 11), kind, 77), f"{kind} (37, 21, 11) uniform noise"
        out.append(_make(kind, vid, vol, "outside", lo=0.3, hi=0.6, spacing=(2, 2, 5)))
        out.append(_make(kind, vid, vol, "close", lo=0.3, hi=0.6, radius=1.0, fill_in=0.45, fill_out=0.0))
        out.append(_make(kind, vid, vol, "erode", lo=-INF, hi=0.2, radius=1.5, fill_in=0.0, fill_out=1.0))
        # the overflow refusal
        vol = LC.percolation(REFUSED, kind, 3)
        out.append(_make(kind, f"{kind} {REFUSED} percolation at density 0.31", vol, "outside", spacing=(64, 64, 64), refused=True))
    # f16: NaN, infinities, zeros of both signs, denormals
    vol, vid = LC.f16_specials((37, 21, 11), 3), "f16 (37, 21, 11) NaN, inf, -0, denormals"
    for j, (lo, hi) in enumerate(((-INF, INF), (0.0, INF), (-INF, 0.0), (0.0, 0.0), (INF, INF), (-INF, -INF), (-1.0, 1.0))):
        out.append(_make("f16", vid, vol, ("outside", "inside")[j % 2], lo=lo, hi=hi, spacing=SPACINGS[j % 3]))
        out.append(_make("f16", vid, vol, MORPH[j % 4], lo=lo, hi=hi, radius=1.5, fill_in=70000.0 if j % 2 else 0.5, fill_out=-0.0))  # 70000: overflows to +inf
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.vol.setflags(write=False)
    _CACHE.extend(out)
    return _CACHE
