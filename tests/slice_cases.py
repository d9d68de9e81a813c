"""The cases of the slice pass (vk_render_slice), shared by tests/test_slice_fuzz_cpu.py (the numpy reference against
the C restatement) and tests/test_slice_fuzz_gpu.py (the kernels against the C restatement).

A case fixes the volume (u8, f16 or R16_UNORM, at most 24^3), the frame (at most 48 x 32), the plane's four vectors as f32, the slab
(samples in {1, 2, 3, 8, 256} under each reduction), the table and its domain (None: the grey ramp), an optional clip box and an optional
tile.  Coverage does not hang on the draw: formats, plane kinds, sample counts, reductions, tables, boxes and tiles are dealt in cycles of
coprime lengths, the draw only fills in their parameters.  The named cases pin the edges: a 1x1x1 volume, planes exactly on the cube's
faces and one ulp outside them, NaN and infinite taps under each reduction, all-NaN slabs, a slab whose samples all clamp, -0 table
entries, half-float output."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import table_cases as TC
import u16_cases as UC

SEED = 20261019
N_RANDOM = 40
SAMPLES = (1, 2, 3, 8, 256)
REDUCE = ("max", "min", "mean")
PLANES = ("oblique", "axis", "oblique", "miss", "du zero", "oblique", "dv zero")
f32 = np.float32


@dataclass
class Case:
    name: str
    vol: np.ndarray             # (nz, ny, nx) u8, f16 or uint16 (R16_UNORM)
    W: int
    H: int
    plane: np.ndarray           # (4, 3) f32: origin, du, dv, dn
    samples: int = 1
    reduce: str = "max"
    table: np.ndarray | None = None  # (n, 4) f32; None: the grey ramp
    domain: tuple = (0.0, 1.0)
    box: tuple | None = None    # (lo3, hi3)
    tile: tuple | None = None   # (tx, ty, tw, th), any origin
    half: bool = False          # also render RGBA16F output
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.vol.shape
        return nx, ny, nz

    @property
    def kind(self):
        return {np.dtype(np.uint8): "u8", np.dtype(np.float16): "f16", np.dtype(np.uint16): "u16"}[self.vol.dtype]

    def __repr__(self):
        return (f"SliceCase({self.name}: dims={self.dims} {self.kind} {self.W}x{self.H} tile={self.tile} samples={self.samples} {self.reduce} "
                f"table={None if self.table is None else self.table.shape[0]} domain={self.domain} box={self.box})")


def _plane(origin, du, dv, dn=(0.0, 0.0, 0.0)):
    return np.array([origin, du, dv, dn], np.float64).astype(np.float32)


def _unit(v):
    return v / np.sqrt((v * v).sum())


def _oblique(rng, W, H, centre, extent, thickness, samples):
    n = _unit(rng.normal(size=3))
    up = rng.normal(size=3)
    up = _unit(up - (up * n).sum() * n)
    right = np.cross(up, n)
    px = extent / W
    du, dv = right * px, -up * px
    dn = n * (thickness / (samples - 1) if samples > 1 else 0.0)
    origin = np.asarray(centre) - 0.5 * (W - 1) * du - 0.5 * (H - 1) * dv
    return _plane(origin, du, dv, dn)


def _axis(rng, dims, W, H, samples):
    """An axis-aligned plane through voxel centres, the frame unrelated to the dims: a little wider than the cube, so its rim misses."""
    axis = int(rng.integers(0, 3))
    a, b = {2: (0, 1), 1: (0, 2), 0: (1, 2)}[axis]
    du, dv, dn, origin = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
    du[a], dv[b] = 1.1 / W, 1.1 / H
    dn[axis] = 1.0 / dims[axis]
    origin[a], origin[b] = -0.05 + 0.55 / W, -0.05 + 0.55 / H
    origin[axis] = (int(rng.integers(0, dims[axis])) + 0.5) / dims[axis]
    return _plane(origin, du, dv, dn)


def _volume(O, rng, kind, dims, finite=False):
    if kind == "u8":
        return TC.u8_standin(O, rng, dims)
    if kind == "f16":
        return TC.f16_finite(O, rng, dims) if finite else TC.f16_edges(O, rng, dims)
    return (UC.vol_a if finite else UC.vol_e)(O, rng, dims)[0]


def _box(rng):
    lo = rng.uniform(0.0, 0.4, 3)
    hi = rng.uniform(0.6, 1.0, 3)
    return tuple(float(f32(v)) for v in lo), tuple(float(f32(v)) for v in hi)


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    out = []
    kinds = ("u8", "f16", "u16")
    ns = (2, 3, 17, 256)
    for trial in range(N_RANDOM):
        kind = kinds[(trial + trial // 15) % 3]  # (samples, reduce) pairs come round every 15 trials: each time in another format
        dims = tuple(int(v) for v in rng.integers(2, 25, 3))
        W, H = int(rng.integers(16, 49)), int(rng.integers(12, 33))
        samples = SAMPLES[trial % len(SAMPLES)]
        reduce = REDUCE[(trial // len(SAMPLES)) % len(REDUCE)]
        pk = PLANES[trial % len(PLANES)]
        thickness = float(rng.choice([0.05, 0.3, 1.5]))
        centre = rng.uniform(0.25, 0.75, 3)
        if pk == "axis":
            plane = _axis(rng, dims, W, H, samples)
        elif pk == "miss":  # wholly outside the cube
            plane = _oblique(rng, W, H, centre + np.array([2.5, -1.5, 3.0]), 0.8, thickness, samples)
        else:
            plane = _oblique(rng, W, H, centre, float(rng.uniform(0.5, 2.2)), thickness, samples)
            if pk == "du zero":
                plane[1] = 0.0
            if pk == "dv zero":
                plane[2] = 0.0
        vol = _volume(O, rng, kind, dims, finite=(reduce == "mean" and trial % 2 == 0))
        table, domain = None, (0.0, 1.0)
        if trial % 4 != 3:
            table = TC.random_table(rng, ns[trial % len(ns)])
            dk = TC.DOMAINS[trial % len(TC.DOMAINS)]
            domain = TC._domain(dk, kind == "f16")
            if kind == "u16" and dk == "narrow":
                domain = (0.3, 0.31)
        box = _box(rng) if trial % 4 == 1 else None
        tile = None
        if trial % 5 == 2:
            tile = (-int(rng.integers(1, 12)), -int(rng.integers(1, 9)), int(rng.integers(20, W + 8)), int(rng.integers(14, H + 6)))
        elif trial % 5 == 4:
            tile = (int(rng.integers(1, 9)), int(rng.integers(1, 7)), int(rng.integers(9, W)), int(rng.integers(7, H)))
        out.append(Case(f"r{trial:02d}", vol, W, H, plane, samples, reduce, table, domain, box, tile, half=(trial in (0, 7)), tags=(pk,)))

    # ---- the named cases ----
    # one voxel: every tap is the same
    out.append(Case("1x1x1", np.full((1, 1, 1), 200, np.uint8), 24, 16, _oblique(rng, 24, 16, (0.5, 0.5, 0.5), 1.4, 0.5, 3), 3, "mean"))
    # planes exactly on the cube's faces: P.x = px / 16, P.y = py / 8, both exact, the corners at 0 and 1; z exactly 0 and exactly 1
    vol = TC.u8_standin(O, rng, (11, 7, 5))
    for z, nm in ((0.0, "z = 0"), (1.0, "z = 1")):
        out.append(Case("on the face " + nm, vol, 17, 9, _plane((0.0, 0.0, z), (1 / 16, 0, 0), (0, 1 / 8, 0)), tags=("face",)))
    # ... and one ulp outside them: every pixel a miss
    below, above = float(np.nextafter(f32(0.0), f32(-1.0))), float(np.nextafter(f32(1.0), f32(2.0)))
    for z, nm in ((below, "below 0"), (above, "above 1")):
        out.append(Case("one ulp outside, " + nm, vol, 17, 9, _plane((0.0, 0.0, z), (1 / 16, 0, 0), (0, 1 / 8, 0)), tags=("ulp",)))
    # NaN and infinite taps in f16 under each reduction: a third of the voxels special, slabs of three across them
    bits = TC.f16_finite(O, rng, (13, 9, 12)).view(np.uint16).copy()
    m = rng.random(bits.shape) < 0.3
    bits[m] = rng.choice(np.array([0x7C00, 0xFC00, 0x7E00, 0x7C01, 0xFC01], np.uint16), int(m.sum()))
    for red in REDUCE:
        out.append(Case("f16 NaN and inf taps, " + red, bits.view(np.float16), 32, 24, _axis(rng, (13, 9, 12), 32, 24, 3), 3, red,
                        TC.random_table(rng, 17), (-0.5, 1.5), tags=("nonfinite",)))
    # all-NaN slabs: MAX stays at -inf (entry 0), MIN at +inf (the last entry)
    nan_vol = np.full((6, 5, 7), 0x7E00, np.uint16).view(np.float16)
    two = np.array([[0.2, 0.4, 0.6, 1.0], [0.9, 0.7, 0.5, 1.0]], np.float32)
    for red in REDUCE:
        out.append(Case("all-NaN slab, " + red, nan_vol, 20, 16, _oblique(rng, 20, 16, (0.5, 0.5, 0.5), 0.6, 0.2, 8), 8, red, two, (0.0, 1.0),
                        tags=("allnan",)))
    # a slab whose samples all clamp: two samples 2.5 cubes either side of the plane
    out.append(Case("every slab sample clamps", _volume(O, rng, "u16", (9, 12, 6), finite=True), 24, 20,
                    _plane((0.05, 0.05, 0.5), (0.9 / 23, 0, 0), (0, 0.9 / 19, 0), (0, 0, 5.0)), 2, "max", tags=("clamps",)))
    # -0 table entries: the colour lerp meets -0 - -0 and fma(f, +-0, -0)
    t = TC.random_table(rng, 17)
    t[3:9, :3] = -0.0
    t[12, 1] = -0.0
    out.append(Case("-0 table entries", TC.u8_standin(O, rng, (20, 18, 16)), 40, 30, _oblique(rng, 40, 30, (0.5, 0.5, 0.5), 1.2, 0.0, 1), 1, "max", t,
                    (0.0, 1.0)))
    # half-float output on a slab under a box
    out.append(Case("rgba16f u16 slab", _volume(O, rng, "u16", (21, 17, 24), finite=True), 48, 32, _oblique(rng, 48, 32, (0.5, 0.5, 0.5), 1.3, 0.2, 8), 8,
                    "mean", TC.random_table(rng, 256), (0.0, 1.0), _box(rng), None, half=True))
    return tuple(out)


N_NAMED = 14


def cases(O):
    """The case list (deterministic: built once from SEED).  O: the oracle module (tests' `O` fixture)."""
    out = _cases(O)
    assert len(out) == N_RANDOM + N_NAMED, len(out)
    return out
