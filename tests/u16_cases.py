"""The seeded cases of the marches on R16_UNORM volumes (VK_FMT_R16_UNORM), shared by tests/test_u16_cpu.py
(the numpy references among themselves) and tests/test_u16_gpu.py (the kernels against the references), so that both walk the same list.

A case fixes the volume (uint16 [nz, ny, nx]), the camera, the frame, dt_scale and the family with its parameters: the built-in transfer,
a table, a lit table, the maximum projection (over a table or the grey ramp) or an isosurface (refine 0 / 4 / 16, lit and unlit), some
under a clip box, some also rendered to RGBA16F.  Dims come from table_cases.FIXED_DIMS (from 1x1x1, straddling cell and brick edges) and
random 5..64, frames are 24..80 px, cameras, dts and lights are table_cases'.  The volumes:
  a   the stand-in widened x257 plus a random low byte ("a0": without the low byte -- the widening cases, whose u8 twin is kept)
  b   12-bit blobs stored unscaled (0..4095); table domains inside [0, 4095/65535]
  c   constants 0, 6553, 6554, 65535: the built-in transfer's empty fractions 1, 1, 0, 0
  d   a 0 / 65535 checker
  e   data holding the words 0x7C00, 0xFC00, 0x7E00 (f16 infinities and NaN) and values >= 0x8000 (negative as i16 or f16)
  f   plateaus of 65535 with iso = 1.0: a hit by equality
Coverage does not hang on the draw: families, volumes and dts are dealt in cycles of coprime lengths.  `noisy` marks the cases whose
frame must change when the low byte of every voxel is dropped (tests/test_u16_cpu.py): every case on the volumes a, b and e, in every
family.  The isosurface cases are seen from close outside cameras (_iso_camera) and are shaded on those volumes, so that the surface fills
enough of the frame and its gradient reads the low bytes."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import table_cases as TC

SEED = 20261020
N_RANDOM = 28
FAMILIES = ("builtin", "table", "lit", "mip", "mipgrey", "iso")
F16_WORDS = (0x7C00, 0xFC00, 0x7E00)


@dataclass
class Case:
    name: str
    vol: np.ndarray             # (nz, ny, nx) uint16
    cam: tuple                  # arguments of oracle.camera_blob
    W: int
    H: int
    dt: float
    family: str                 # one of FAMILIES
    table: np.ndarray | None = None
    domain: tuple = (0.0, 1.0)
    light: dict | None = None   # keyword arguments of Context.set_lighting (lit; iso: lit when given)
    iso: float | None = None
    refine: int = 4
    colour: tuple = (0.9, 0.7, 0.3)
    box: tuple | None = None    # (lo3, hi3)
    half: bool = False          # also render RGBA16F output
    noisy: bool = False
    u8: np.ndarray | None = None  # the widening cases: the u8 volume this one is x257 of
    empty: float | None = None  # the PACKED layout's built-in empty fraction this case must report
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.vol.shape
        return nx, ny, nz

    @property
    def lit(self):
        return self.light is not None and self.family in ("lit", "iso")

    def __repr__(self):
        return (f"U16Case({self.name}: {self.family} vol={self.tags} dims={self.dims} {self.W}x{self.H} dt={self.dt} box={self.box} "
                f"iso={self.iso} refine={self.refine} lit={self.lit})")


# ---- volumes ----

def vol_a0(O, rng, dims):
    v8 = TC.u8_standin(O, rng, dims)
    return v8.astype(np.uint16) * np.uint16(257), v8


def vol_a(O, rng, dims):
    v, _ = vol_a0(O, rng, dims)
    low = rng.integers(0, 256, v.shape)
    return np.minimum(v.astype(np.int64) + low, 65535).astype(np.uint16), None


def vol_b(O, rng, dims):
    v = TC._blobs(rng, dims, 0.0, (1500.0, 4095.0)) + rng.integers(0, 300, dims[::-1])
    return np.clip(v, 0, 4095).astype(np.uint16), None


def vol_d(O, rng, dims):
    z, y, x = TC._grid(dims)
    return np.where((x + y + z) % 2 == 0, 0, 65535).astype(np.uint16), None


def vol_e(O, rng, dims):
    """Smooth blobs over the whole range with 10 % of the voxels replaced by f16 infinity / NaN words and by values >= 0x8000."""
    v = np.clip(TC._blobs(rng, dims, 2000.0, (30000.0, 65535.0)) + rng.integers(0, 3000, dims[::-1]), 0, 65535).astype(np.uint16)
    specials = np.array(F16_WORDS + (0x8000, 0x8001, 0xBC00, 0xFFFF, 0xFBFF), np.uint16)
    m = rng.random(v.shape) < (0.1 if min(dims) > 2 else 0.5)
    v[m] = rng.choice(specials, int(m.sum()))
    if v.size >= 4:
        v.flat[rng.choice(v.size, 4, replace=False)] = specials[:4]
    return v, None


def vol_f(O, rng, dims):
    """Plateaus of 65535 (boxes a third to two thirds of the volume wide) in a low background: inside one a sample is 65535 exactly."""
    v = rng.integers(0, 20000, dims[::-1]).astype(np.uint16)
    nx, ny, nz = dims
    for _ in range(4):
        sz = [max(2, int(rng.integers(n // 3, 2 * n // 3 + 1))) for n in (nz, ny, nx)]
        lo = [int(rng.integers(0, max(1, n - s + 1))) for n, s in zip((nz, ny, nx), sz)]
        v[lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = 65535
    return v, None


VOLUMES = {"a": vol_a, "b": vol_b, "d": vol_d, "e": vol_e, "f": vol_f, "a0": vol_a0}
NOISY = ("a", "b", "e")
# what an isosurface / a table's window is set to on each kind of volume (sample values: t / 65535).  On the noisy volumes the threshold sits
# just above a multiple of 256 and well inside the data: with the low bytes dropped the surface lies where the data reaches the next multiple
ISO_OF = {"a": 0x7310 / 65535.0, "a0": 0.45, "b": 0x0310 / 65535.0, "d": 0.5, "e": 0x4010 / 65535.0, "f": 1.0}
DOMAIN_OF = {"a": (0.0, 1.0), "a0": (0.0, 1.0), "b": (100.0 / 65535.0, 4095.0 / 65535.0), "d": (0.0, 1.0), "e": (0.05, 0.95), "f": (0.0, 1.0)}


def _iso_camera(rng, kind, W, H):
    """A surface is looked at from outside and from near enough to fill the frame: a close orbit (even kinds) or a close axis-aligned view,
    whose centre rays have direction components that are exactly zero (odd kinds)."""
    if kind % 2 == 0:
        return (float(rng.uniform(0.6, 0.9)), float(rng.uniform(-1.2, 1.2)), float(rng.uniform(0, 6.28)), (0.5, 0.5, 0.5), W / H)
    return (0.9, 0.0, float(rng.integers(0, 4)) * 1.5707963, (0.5, 0.5, 0.5), 1.0)


def _box(rng):
    lo = tuple(float(v) for v in rng.uniform(0.0, 0.35, 3))
    hi = tuple(float(v) for v in rng.uniform(0.65, 1.0, 3))
    return lo, hi


def _table(rng, family, n):
    t = TC.random_table(rng, n)
    if family in ("table", "lit"):
        t[:, 3] = np.where(t[:, 3] == 0.0, t[:, 3], np.maximum(t[:, 3], 0.02))  # (faint, but a frame's colour is well above the bars)
    return t


def _make(O, rng, name, family, vkind, dims, W, H, dt, cam_kind, *, box=False, half=False, refine=4, iso_lit=True):
    vol, u8 = VOLUMES[vkind](O, rng, dims)
    if vol.size == 1 and vkind == "a":
        vol[...] = 0x6AC7  # (one voxel: a mid-range value with a large low byte, whatever the draw)
    cam = _iso_camera(rng, cam_kind, W, H) if family == "iso" else TC._camera(rng, cam_kind, W, H)
    c = Case(name, vol, cam, W, H, dt, family, u8=u8, tags=(vkind,))
    if family in ("table", "lit", "mip"):
        c.table = _table(rng, family, (256, 17, 3, 64)[int(rng.integers(0, 4))])
        c.domain = DOMAIN_OF[vkind]
    if family == "lit" or (family == "iso" and (iso_lit or vkind in NOISY)):  # (on a noisy volume the isosurface is shaded: its gradient reads the low bytes)
        c.light = TC._light(O, rng, ("headlight", "random", "+x", "view")[int(rng.integers(0, 4))], cam)
        if c.light["ambient"] == 0.0 and c.light["diffuse"] == 0.0:
            c.light["ambient"] = 0.25  # (a light at its bounds with nothing but a pin-point highlight leaves the frame black)
    if family == "iso":
        c.iso, c.refine = ISO_OF[vkind], refine
    if box and family != "builtin":
        c.box = _box(rng)
    c.half = half
    # a dropped low byte must show, in every family (_cases deals the built-in transfer no 12-bit volume: all of it lies below its threshold)
    c.noisy = vkind in NOISY
    assert not (family == "builtin" and vkind == "b")
    return c


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    out = []
    vkinds = ("a", "b", "e", "f", "d")
    dts = (0.15, 0.5, 1.0, 1.7, 0.5, 3.5, 0.013)
    refines = (0, 4, 16)
    for trial in range(N_RANDOM):
        family = FAMILIES[trial % len(FAMILIES)]
        vkind = vkinds[trial % len(vkinds)]
        if family == "builtin" and vkind == "b":
            vkind = "a"
        dt = dts[trial % len(dts)]
        hi = 14 if dt < 0.1 else 64
        dims = tuple(int(x) for x in rng.integers(5, hi + 1, 3))
        W, H = int(rng.integers(24, 81)), int(rng.integers(24, 81))
        if dt < 0.1:
            W, H = min(W, 40), min(H, 40)
        cam_kind = trial % 4  # (the isosurface cases: _iso_camera)
        out.append(_make(O, rng, f"r{trial:02d}", family, vkind, dims, W, H, dt, cam_kind, box=trial % 5 in (1, 2), half=trial % 9 == 4,
                         refine=refines[(trial // len(FAMILIES)) % 3], iso_lit=(trial // len(FAMILIES)) % 2 == 0))
    # dims from 1x1x1, straddling the cell (4) and brick edges, one family each
    for j, dims in enumerate(TC.FIXED_DIMS):
        family = ("builtin", "iso", "table", "mip", "lit")[j]
        out.append(_make(O, rng, "dims" + "x".join(map(str, dims)), family, ("a", "f", "e", "b", "a")[j], dims, 40, 32, (0.5, 1.0, 0.15, 0.5, 1.7)[j],
                         0, box=j == 4, refine=16))
    # the widening cases: x257 of a u8 stand-in, no noise, one per family; the u8 references must give the same steps
    for j, family in enumerate(FAMILIES):
        out.append(_make(O, rng, "widen " + family, family, "a0", (33, 29, 37), 48, 40, 0.5, 0, half=j == 1))
    # constants at the built-in threshold: 6553 is the last empty tap, 6554 the first that is not
    for value, ef in ((0, 1.0), (6553, 1.0), (6554, 0.0), (65535, 0.0)):
        c = Case(f"constant {value}", np.full((11, 9, 13), value, np.uint16), TC._camera(rng, 0, 32, 24), 32, 24, 0.5, "builtin", empty=ef, tags=("c",))
        out.append(c)
    # the isosurface at the top of the range, a hit by equality, unlit and lit, and one under a box with half-float output
    out.append(_make(O, rng, "plateaus iso 1.0 unlit", "iso", "f", (21, 18, 26), 48, 36, 0.5, 0, refine=0, iso_lit=False))
    out.append(_make(O, rng, "plateaus iso 1.0 lit box", "iso", "f", (30, 17, 22), 48, 36, 1.0, 0, box=True, half=True, refine=16))
    # the checker under the built-in transfer and the grey ramp: every cell holds both extremes
    out.append(_make(O, rng, "checker builtin", "builtin", "d", (9, 12, 7), 40, 32, 0.5, 0))
    out.append(_make(O, rng, "checker grey ramp", "mipgrey", "d", (13, 8, 10), 40, 32, 1.0, 1))
    return tuple(out)


N_CASES = N_RANDOM + len(TC.FIXED_DIMS) + len(FAMILIES) + 4 + 4


def cases(O):
    out = _cases(O)
    assert len(out) == N_CASES, len(out)
    return out


_REF = {}


def reference(O, c, vol=None):
    """The case's reference frame, computed once per case and kept: (rgb float64 [H, W, 3], steps u32 [H, W], nonempty u32 [H, W] or None).
    vol: another volume in the case's place (not kept)."""
    import np_u16_reference as NU

    key = c.name if vol is None else None
    if key in _REF:
        return _REF[key]
    v = c.vol if vol is None else vol
    cam = O.camera_blob(*c.cam)
    if c.family == "builtin":
        rgb, steps, live = NU.render_builtin(cam, v, c.W, c.H, dt=c.dt)
    elif c.family in ("table", "lit"):
        rgb, steps = NU.render_table(c.box, cam, v, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt, light=c.light if c.family == "lit" else None)
        live = None
    elif c.family in ("mip", "mipgrey"):
        rgb, steps, live = NU.render_mip(c.box, cam, v, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt)
    else:
        rgb, steps, live = NU.render_iso(c.box, cam, v, c.W, c.H, iso=c.iso, colour=c.colour, refine=c.refine, dt=c.dt, light=c.light)[:3]
    if key is not None:
        _REF[key] = (rgb, steps, live)
    return rgb, steps, live
