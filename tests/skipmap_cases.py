"""The volumes and states the skip maps are read back under (tests/test_skipmap_cpu.py holds the list to its conditions,
tests/test_skipmap_gpu.py compares every byte of every map with tests/np_skipmap_reference.py).  Small volumes chosen for the map
builders, not for pictures:

  long      113 x 6 x 5, 7 x 109 x 9 and 5 x 6 x 121 in u8, f16 and u16: a blob near one end, a blob in the middle, two blobs whose nearest
            non-empty cells are 49, 50 and 51 cells apart (the windows of the two just meet, touch and miss), an empty volume (every byte
            25) and a full one -- distances beyond 13, the window |j| <= 24, the clamp to 25, windows cut at the far grid edge, and the
            bricked order at up to 32 bricks per axis
  gap       700 x 1 x 2, full but for one run of 51 empty cells: the only way to a 25 in an ISOTROPIC map (under 30 % empty)
  edges     1 x 1 x 1, 33 x 20 x 7, dimensions of 4k, 4k + 1 and 4k + 3, and the 40 x 36 x 44 speckle volume of test_speckle_skip_gpu.py with
            its all-255 variant (the codes)
  lopsided  material in one corner only, and in a patch of one face only
  share     three volumes on a grid of 5 x 2 x 2 bricks (1280 cells) with exactly 384 (30 %), 383 and 385 empty cells, found by search
  values    f16 with NaN, +-inf and taps on both sides of 0.1, u8 on 25 / 26, u16 on 6553 / 6554
  records   RGBA16F_PAIR volumes for the embedded record map: 250 x 4 x 4 (a distance of 61 is reached) and 9 x 6 x 5

Every volume is read under each of its states: the built-in transfer, the band-pass table, the inverted table of table_cases.py, the
maximum projection over the band-pass table and over the grey ramp, and an isosurface inside and above the data.  The blob volumes are
air of 0 with blobs of 0.62 (u8 158, u16 158 * 257): non-empty under the built-in transfer, inside the band of the band-pass table over
the tables' domain (0.25, 0.9), clear under the inverted table, above the threshold 0.3."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import builtin_cases as BC
import np_skipmap_reference as SK
import table_cases as TC
import u16_cases as UC
from tf_helpers import band_pass_table

SEED = 20261019
DOMAIN = (0.25, 0.9)
STATES = ("builtin", "band", "inverted", "max table", "max grey", "iso in", "iso above")
FEW_STATES = ("builtin", "band", "iso in")  # the larger volumes
BAND = band_pass_table()
INVERTED = TC.inverted_table(np.random.default_rng(SEED), 64)
LONG_DIMS = {"x": (113, 6, 5), "y": (7, 109, 9), "z": (5, 6, 121)}
SHARE_DIMS = (16, 4, 4)     # 5 x 2 x 2 bricks
SHARE_EMPTY = 384           # 30 % of 1280 cells
MIN_TOTAL_CELLS = 50_000_000 # cells of all maps of all (volume, state) pairs: see test_skipmap_cpu.py


@dataclass
class Case:
    name: str
    vol: np.ndarray             # (nz, ny, nx) u8, f16 or u16 (R16_UNORM)
    kind: str                   # long, gap, edges, lopsided, share, values
    iso_in: float = 0.3         # a threshold inside the data, in sample values
    iso_above: float = 2.0      # and one above every finite value
    states: tuple = STATES
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.vol.shape
        return nx, ny, nz

    @property
    def fmt(self):
        return SK.fmt_of(self.vol)

    def __repr__(self):
        return f"SkipCase({self.name}: {self.kind} {self.fmt} dims={self.dims} {self.tags})"


def state_of(c, name):
    """The state dict np_skipmap_reference.seed_empty takes (None: the built-in transfer)."""
    return {"builtin": None,
            "band": {"table": BAND, "domain": DOMAIN},
            "inverted": {"table": INVERTED, "domain": DOMAIN},
            "max table": {"table": BAND, "domain": DOMAIN, "mip": True},
            "max grey": {"mip": True},
            "iso in": {"iso": c.iso_in},
            "iso above": {"iso": c.iso_above}}[name]


def family_of(name):
    """Which of cell_occ_kernel's predicates a state seeds the maps with."""
    return {"builtin": "built-in", "band": "table", "inverted": "table", "max table": "max", "max grey": "max", "iso in": "iso", "iso above": "iso"}[name]


# ---- material ----

def as_fmt(mask, fmt):
    """Air of 0 with 0.62 where `mask` is set."""
    if fmt == "u8":
        return np.where(mask, 158, 0).astype(np.uint8)
    if fmt == "u16":
        return np.where(mask, 158 * 257, 0).astype(np.uint16)
    return np.where(mask, 0.62, 0.0).astype(np.float16)


def _long_masks(axis):
    nx, ny, nz = LONG_DIMS[axis]
    a = {"x": 2, "y": 1, "z": 0}[axis]   # the array axis
    n = (nz, ny, nx)[a]

    def blob(m, at):
        """A 2-voxel-thick blob: its non-empty cells are those of low-corner voxels at - 1 .. at + 1 on the long axis."""
        sl = [slice(1, 3)] * 3
        sl[a] = slice(at, at + 2)
        m[tuple(sl)] = True

    out = {}
    for name, ats in (("end", (3,)), ("middle", (n // 2,)), ("apart 49", (10, 61)), ("apart 50", (10, 62)), ("apart 51", (10, 63))):
        m = np.zeros((nz, ny, nx), bool)
        for at in ats:
            blob(m, at)
        out[name] = m
    out["empty"] = np.zeros((nz, ny, nx), bool)
    out["full"] = np.ones((nz, ny, nx), bool)
    return out


def _share_volumes():
    """Fill the SHARE_DIMS volume voxel by voxel in a drawn order until exactly SHARE_EMPTY, SHARE_EMPTY - 1 and SHARE_EMPTY + 1 cells are
    empty under the reference seed (the count falls as voxels are filled: bisection over the order's prefixes; orders are drawn until each of
    the three counts has been met)."""
    nx, ny, nz = SHARE_DIMS
    want = {SHARE_EMPTY: None, SHARE_EMPTY - 1: None, SHARE_EMPTY + 1: None}
    for s in range(400):
        order = np.random.default_rng(SEED + s).permutation(nx * ny * nz)

        def filled(k):
            m = np.zeros(nx * ny * nz, bool)
            m[order[:k]] = True
            return m.reshape(nz, ny, nx)

        def empties(k):
            return int(SK.seed_empty(as_fmt(filled(k), "u8")).sum())

        for target in [t for t, v in want.items() if v is None]:
            lo, hi = 0, order.size  # the smallest prefix with at most `target` empty cells
            while lo < hi:
                mid = (lo + hi) // 2
                if empties(mid) <= target:
                    hi = mid
                else:
                    lo = mid + 1
            if empties(lo) == target:
                want[target] = filled(lo)
        if all(v is not None for v in want.values()):
            return want
    raise AssertionError("no filling order met the three empty counts")


def _speckle_volume(hot_all_255=False):
    from test_speckle_skip_gpu import _volume

    return _volume(hot_all_255)


def _u16_threshold(rng, dims):
    """Air of 6553 (the largest empty tap) with lone 6554 speckles and one blob: the u16 twin of builtin_cases.u8_speckle."""
    vol = np.full(dims[::-1], 6553, np.uint16)
    vol[rng.random(vol.shape) < 0.004] = 6554
    vol.flat[int(rng.integers(0, vol.size))] = 6554
    vol[2:5, 3:6, 4:8] = 40000
    return vol


def _cases():
    rng = np.random.default_rng(SEED)
    out = []
    for axis in LONG_DIMS:
        for cname, mask in _long_masks(axis).items():
            for fmt in ("u8", "f16", "u16"):
                out.append(Case(f"long {axis} {cname} {fmt}", as_fmt(mask, fmt), "long", tags=(axis, cname)))
    gap = np.ones((2, 1, 700), bool)
    gap[:, :, 300:352] = False   # voxels 300 .. 351 are air: the cells of low-corner voxels 300 .. 350 are empty, 51 of them
    out.append(Case("gap u8", as_fmt(gap, "u8"), "gap", states=("builtin", "max grey", "iso in")))
    out.append(Case("gap u16", as_fmt(gap, "u16"), "gap", states=("builtin", "band")))

    for fmt in ("u8", "f16", "u16"):
        out.append(Case(f"1x1x1 air {fmt}", as_fmt(np.zeros((1, 1, 1), bool), fmt), "edges"))
        out.append(Case(f"1x1x1 dense {fmt}", as_fmt(np.ones((1, 1, 1), bool), fmt), "edges"))
    for dims in ((33, 20, 7), (8, 12, 4), (9, 5, 13), (11, 7, 15)):
        out.append(Case(f"{dims} u8 blobs", TC.u8_blobs(None, rng, dims), "edges", iso_in=0.4))
        out.append(Case(f"{dims} f16 edges", TC.f16_edges(None, rng, dims), "edges", iso_in=0.4))
        out.append(Case(f"{dims} u16 plateaus", UC.vol_f(None, rng, dims)[0], "edges", iso_in=0.5))
    out.append(Case("speckle volume", _speckle_volume(), "edges", iso_in=0.4, states=FEW_STATES, tags=("codes",)))
    out.append(Case("speckle volume, all 255", _speckle_volume(True), "edges", iso_in=0.4, states=("builtin",), tags=("codes",)))

    dims = (21, 14, 10)
    corner = np.zeros(dims[::-1], bool)
    corner[:3, :3, :3] = True
    patch = np.zeros(dims[::-1], bool)
    patch[2:6, 3:8, 0] = True   # on the face x = 0
    for fmt in ("u8", "f16", "u16"):
        out.append(Case(f"corner {fmt}", as_fmt(corner, fmt), "lopsided"))
        out.append(Case(f"face patch {fmt}", as_fmt(patch, fmt), "lopsided"))

    for n_empty, mask in sorted(_share_volumes().items()):
        for fmt in ("u8", "f16", "u16"):
            out.append(Case(f"share {n_empty} of 1280 {fmt}", as_fmt(mask, fmt), "share", states=("builtin", "band", "max table", "iso in"), tags=(n_empty,)))

    vdims = (23, 18, 11)
    out.append(Case("f16 edge values", BC.f16_edges(None, rng, vdims), "values", iso_in=0.5))
    out.append(Case("f16 thresholds", BC.f16_thresholds(None, rng, vdims), "values", iso_in=0.5))
    out.append(Case("f16 non-finite ball", BC.f16_nonfinite_ball(None, rng, vdims), "values", iso_in=0.5))
    out.append(Case("u8 25 / 26", BC.u8_speckle(None, rng, vdims), "values", iso_in=26.0 / 255.0))
    out.append(Case("u16 6553 / 6554", _u16_threshold(rng, vdims), "values", iso_in=6554.0 / 65535.0))
    out.append(Case("u16 specials", UC.vol_e(None, rng, vdims)[0], "values", iso_in=0.5))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _cases()
    return _CASES


# ---- records ----

@dataclass
class RecordCase:
    name: str
    den: np.ndarray   # f16 [nz, ny, nx, 4]: colour, opacity
    nrm: np.ndarray   # f16 [nz, ny, nx, 4]

    @property
    def dims(self):
        nz, ny, nx = self.den.shape[:3]
        return nx, ny, nz


def record_cases():
    rng = np.random.default_rng(SEED + 1)
    out = []
    for name, dims in (("records 250x4x4", (250, 4, 4)), ("records 9x6x5", (9, 6, 5))):
        nx, ny, nz = dims
        den = np.zeros((nz, ny, nx, 4), np.float16)
        den[..., :3] = rng.uniform(0.0, 1.0, (nz, ny, nx, 3))
        nrm = rng.uniform(-1.0, 1.0, (nz, ny, nx, 4)).astype(np.float16)
        den[1:3, 1:3, 2:4, 3] = 0.8          # the one blob, near the low end of x
        den[0, 0, 0, 3] = np.float16(1e-3)     # a faint record is not an empty one
        den[3, 0, 8, 3] = np.float16(2.0 ** -24)  # nor is the smallest f16 subnormal: s * s = 4.6e-43 is an f32 subnormal, not 0
        den[0, 1, 5, 3] = np.nan               # a NaN opacity is 0
        den[0, 2, 6, 3] = -0.5
        if nx > 100:
            den[3, 3, 12, 0] = np.inf         # an infinite colour contributes NaN: not empty
            nrm[2, 0, 20, 1] = -np.inf        # so does a -inf normal component
            nrm[1, 1, 30, 2] = np.inf          # +inf is harmless
            nrm[1, 2, 31, 0] = np.nan
        out.append(RecordCase(name, den, nrm))
    return out
