"""The seeded fuzz cases of the built-in transfer function (VK_MODE_NAIVE_TRILINEAR, no table), shared by tests/test_builtin_fuzz_cpu.py
(the numpy reference against the C oracle, the skip-map predicate sample by sample) and tests/test_builtin_fuzz_gpu.py (every layout
against the oracle), so that both walk the same list.

Each case fixes the volume (u8 or f16), the camera (the four kinds of tests/table_cases.py), the image and an optional tile, dt_scale and
the empty fraction the volume is built for.  The kinds of volume, camera and dt are dealt in cycles of coprime lengths (7, 4, 6); the draw
only fills in their parameters.  The volumes carry the values where the built-in transfer and its skip maps can go wrong: f16 +-0,
subnormals, negatives down to -65504, both sides of the 0.1 threshold and of the 0.9 clamp, 1.0, 65504, +-inf and NaN bit patterns; u8 25
next to 26, 0 next to 255 (PACKED_PAIRS deltas of +-255) and saturated blocks.  Dims straddle the 4-voxel cells, the 9^3 bricks, the
9x8x8 quads and the staged 8^3 bricks."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from table_cases import _camera

SEED = 20261017
DTS = (0.013, 0.15, 0.5, 1.0, 1.7, 3.5)
N_RANDOM = 35
FIXED_DIMS = ((1, 1, 1), (2, 3, 5), (4, 4, 4), (5, 4, 9), (8, 8, 8), (9, 9, 9), (17, 8, 33), (1, 40, 7))
# f16 edge values as bit patterns
F16_NAN_BITS = (0x7E00, 0x7C01, 0xFC01, 0xFE00)
F16_EDGE_BITS = {
    "+0": 0x0000, "-0": 0x8000, "smallest subnormal": 0x0001, "largest subnormal": 0x03FF, "-smallest subnormal": 0x8001,
    "-1": 0xBC00, "-0.6": 0xB8CD, "-65504": 0xFBFF,
    "0.09998": 0x2E66, "0.10004": 0x2E67, "0.8999": 0x3B33, "0.9004": 0x3B34, "1.0": 0x3C00, "65504": 0x7BFF,
    "+inf": 0x7C00, "-inf": 0xFC00, **{f"NaN {b:#06x}": b for b in F16_NAN_BITS},
}
# empty under the built-in predicate (finite and <= 0.1): the air the f16 volumes are made of
F16_EMPTY_BITS = (0x0000, 0x8000, 0x0001, 0x03FF, 0x8001, 0xBC00, 0xB8CD, 0xFBFF, 0x2E66, 0x2519)  # (0x2519: 0.02)
F16_NONFINITE_BITS = (0x7C00, 0xFC00) + F16_NAN_BITS
U8_EDGES = (0, 25, 26, 254, 255)


@dataclass
class Case:
    name: str
    vol: np.ndarray             # (nz, ny, nx) u8 or f16
    cam: tuple                  # arguments of oracle.camera_blob: zoom, pitch, yaw, target, aspect
    kind: int                   # the camera kind: 0 orbit, 1 eye inside, 2 axis-aligned, 3 grazing a face
    W: int
    H: int
    dt: float
    tile: tuple | None = None   # (tx, ty, tw, th), any origin
    empty: float | None = None  # the packed layouts' empty fraction this case is built for
    half: bool = False          # also render RGBA16F output
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.vol.shape
        return nx, ny, nz

    @property
    def f16(self):
        return self.vol.dtype == np.float16

    @property
    def edge(self):
        """An edge case of the skip maps: an f16 volume with non-finite or threshold taps, or a u8 volume on the 25/26 threshold."""
        return "edge" in self.tags

    def __repr__(self):
        return (f"Case({self.name}: dims={self.dims} {'f16' if self.f16 else 'u8'} {self.W}x{self.H} tile={self.tile} dt={self.dt} "
                f"camera kind {self.kind} empty={self.empty})")


def _grid(dims):
    nx, ny, nz = dims
    return np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")


def _balls(rng, dims, count):
    """Boolean masks of `count` random balls (radius >= 1 voxel)."""
    z, y, x = _grid(dims)
    out = []
    for _ in range(count):
        c = rng.uniform(0.15, 0.85, 3) * np.array(dims)
        rad = rng.uniform(1.0, max(1.5, 0.35 * min(dims)))
        out.append((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 < rad * rad)
    return out


def _sprinkle(rng, bits, values, p):
    """Set a share p of the voxels to values drawn from `values`, and each value at least once where the volume is large enough."""
    m = rng.random(bits.shape) < p
    bits[m] = rng.choice(np.array(values, np.uint16), int(m.sum()))
    if bits.size >= 4 * len(values):
        bits.flat[rng.choice(bits.size, len(values), replace=False)] = values
    return bits


def _air16(rng, dims):
    """f16 air: every tap empty (finite and <= 0.1), drawn from F16_EMPTY_BITS and 0.02 +- noise."""
    shape = dims[::-1]
    air = (0.02 + rng.uniform(-0.02, 0.05, shape)).astype(np.float16).view(np.uint16)
    pick = rng.random(shape) < 0.5
    air[pick] = rng.choice(np.array(F16_EMPTY_BITS, np.uint16), int(pick.sum()))
    return air


def f16_edges(O, rng, dims):
    """Finite blobs in f16 air, every edge value sprinkled in."""
    bits = _air16(rng, dims)
    for ball in _balls(rng, dims, 3):
        bits[ball] = rng.uniform(0.05, 1.3, int(ball.sum())).astype(np.float16).view(np.uint16)
    return _sprinkle(rng, bits, tuple(F16_EDGE_BITS.values()), 0.03 if min(dims) > 2 else 0.3).view(np.float16)


def f16_thresholds(O, rng, dims):
    """Air of 0x2E66 (0.09998: empty) with lone 0x2E67 (0.10004) speckles, and blobs of the values on both sides of the 0.9 clamp, 1.0
    and 65504."""
    bits = np.full(dims[::-1], 0x2E66, np.uint16)
    for ball in _balls(rng, dims, 2):
        bits[ball] = rng.choice(np.array([0x2E67, 0x3B33, 0x3B34, 0x3C00, 0x7BFF], np.uint16), int(ball.sum()))
    return _sprinkle(rng, bits, (0x2E67,), 0.004).view(np.float16)


def f16_nonfinite_ball(O, rng, dims):
    """f16 air with one ball of a non-finite value (-inf, +inf or a NaN pattern) and a finite blob."""
    bits = _air16(rng, dims)
    a, b = _balls(rng, dims, 2)
    bits[b] = rng.uniform(0.1, 1.0, int(b.sum())).astype(np.float16).view(np.uint16)
    bits[a] = rng.choice(np.array(F16_NONFINITE_BITS, np.uint16))
    return bits.view(np.float16)


def u8_speckle(O, rng, dims):
    """Air of 25 (empty) with lone 26 speckles (the smallest value that is not)."""
    vol = np.full(dims[::-1], 25, np.uint8)
    m = rng.random(vol.shape) < 0.004
    vol[m] = 26
    vol.flat[int(rng.integers(0, vol.size))] = 26
    return vol


def u8_checker(O, rng, dims):
    """0/255 voxel checkerboard (PACKED_PAIRS deltas of +-255) in a box, 0 around it; the phase is drawn."""
    z, y, x = _grid(dims)
    vol = (((x + y + z + int(rng.integers(0, 2))) & 1) * 255).astype(np.uint8)
    lo = [int(rng.integers(0, max(1, d // 3))) for d in dims]
    box = (x >= lo[0]) & (y >= lo[1]) & (z >= lo[2])
    return np.where(box, vol, 0).astype(np.uint8)


def u8_saturated(O, rng, dims):
    """Blocks of 254 and 255 (alpha at its clamp: rays end early) in air of 0..25."""
    vol = rng.integers(0, 26, dims[::-1]).astype(np.uint8)
    for _ in range(3):
        lo = [int(rng.integers(0, d)) for d in dims]
        hi = [lo[k] + int(rng.integers(1, max(2, dims[k] // 2 + 1))) for k in range(3)]
        vol[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = rng.choice(np.array([254, 255], np.uint8))
    return vol


def u8_standin_or_fog(O, rng, dims):
    if rng.random() < 0.5:
        return O.volume_fog_u8(dims, seed=int(rng.integers(1, 1 << 30)), lo=int(rng.integers(18, 27)), span=int(rng.integers(4, 30)))
    if min(dims) >= 17:
        return O.volume_standin_u8(dims, seed=int(rng.integers(1, 1 << 30)))
    return rng.integers(0, 60, dims[::-1]).astype(np.uint8)


VOLUMES = {"f16 edges": f16_edges, "u8 speckle": u8_speckle, "f16 thresholds": f16_thresholds, "u8 checker": u8_checker,
           "f16 non-finite ball": f16_nonfinite_ball, "u8 saturated": u8_saturated, "u8 stand-in or fog": u8_standin_or_fog}
EDGE_KINDS = ("f16 edges", "f16 thresholds", "f16 non-finite ball", "u8 speckle")


def _random_dims(rng, hi):
    """3 .. hi per axis, two axes in three on either side of a multiple of 4 or 8 (cells, 9^3 bricks, 9x8x8 quads, staged 8^3 bricks)."""
    near = [v for v in range(3, hi + 1) if (v % 4) in (1, 3) or (v % 8) in (1, 7)]
    return tuple(int(rng.choice(near)) if rng.random() < 0.67 else int(rng.integers(3, hi + 1)) for _ in range(3))


def _ball(dims, value_bits, air_bits=0x2519, frac=0.3):
    """A ball of value_bits (radius frac * min(dims)) in the middle of f16 air of air_bits."""
    z, y, x = _grid(dims)
    c = (np.array(dims) - 1) / 2.0
    rad = max(1.0, frac * min(dims))
    bits = np.full(x.shape, air_bits, np.uint16)
    bits[(x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 < rad * rad] = value_bits
    return bits.view(np.float16)


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    cases = []
    vkinds = tuple(VOLUMES)
    for trial in range(N_RANDOM):
        dt = DTS[trial % len(DTS)]
        vkind = vkinds[trial % len(vkinds)]
        kind = trial % 4
        hi_dims = 16 if dt < 0.1 else 72  # (the smallest step: ~2000 iterations per ray over 16 cells)
        dims = _random_dims(rng, hi_dims)
        W, H = int(rng.integers(24, 97)), int(rng.integers(24, 97))
        if dt < 0.1:
            W, H = min(W, 40), min(H, 40)
        cam = _camera(rng, kind, W, H)
        vol = VOLUMES[vkind](O, rng, dims)
        tags = (vkind, "random dims") + (("edge",) if vkind in EDGE_KINDS else ())
        cases.append(Case(f"r{trial:02d}", vol, cam, kind, W, H, dt, half=trial % 9 == 4, tags=tags))
    # dims that straddle the cells, the bricks, the quads and the staged bricks; volumes of one voxel and of one voxel per axis
    for j, dims in enumerate(FIXED_DIMS):
        vkind = vkinds[(3 * j + 1) % len(vkinds)]
        W, H = (40, 32) if j % 2 else (33, 41)
        cam = _camera(rng, j % 4, W, H)
        tags = (vkind, "fixed dims") + (("edge",) if vkind in EDGE_KINDS else ())
        cases.append(Case(f"dims{'x'.join(map(str, dims))}", VOLUMES[vkind](O, rng, dims), cam, j % 4, W, H, DTS[(j + 2) % len(DTS)], tags=tags))
    # the named f16 cases: balls of -inf, NaN, +inf in air; -inf everywhere; air of -0, subnormals and negatives only
    d = (32, 32, 32)
    cam = _camera(rng, 0, 48, 40)
    cases.append(Case("-inf ball in air", _ball(d, 0xFC00), cam, 0, 48, 40, 0.5, tags=("edge",)))
    nan = _ball(d, 0x7E00).view(np.uint16).copy()
    m = nan == 0x7E00
    nan[m] = rng.choice(np.array(F16_NAN_BITS, np.uint16), int(m.sum()))
    cases.append(Case("NaN ball in air", nan.view(np.float16), _camera(rng, 1, 44, 44), 1, 44, 44, 1.0, tags=("edge",)))
    cases.append(Case("+inf ball in air", _ball((27, 33, 21), 0x7C00), _camera(rng, 2, 40, 40), 2, 40, 40, 0.15, half=True, tags=("edge",)))
    cases.append(Case("-inf throughout", np.full((13, 11, 19), 0xFC00, np.uint16).view(np.float16), _camera(rng, 0, 36, 30), 0, 36, 30, 1.7,
                      empty=0.0, tags=("edge",)))
    air = rng.choice(np.array([0x8000, 0x0001, 0x03FF, 0x8001, 0xBC00, 0xB8CD, 0xFBFF, 0x0000], np.uint16), (23, 29, 17))
    cases.append(Case("air of -0, subnormals and negatives", air.view(np.float16), _camera(rng, 3, 40, 36), 3, 40, 36, 0.5, empty=1.0,
                      tags=("edge",)))
    # the named u8 cases: the threshold everywhere, and the volumes of the parity suite
    cases.append(Case("all 25", np.full((21, 18, 25), 25, np.uint8), _camera(rng, 0, 40, 32), 0, 40, 32, 1.0, empty=1.0, tags=("edge",)))
    cases.append(Case("all 26", np.full((19, 26, 17), 26, np.uint8), _camera(rng, 1, 40, 32), 1, 40, 32, 0.5, empty=0.0, tags=("edge",)))
    cases.append(Case("25 air, lone 26 speckles", u8_speckle(O, rng, (41, 37, 33)), _camera(rng, 0, 56, 48), 0, 56, 48, 0.5, half=True,
                      tags=("edge",)))
    cases.append(Case("0/255 checkerboard", u8_checker(O, rng, (24, 31, 28)), _camera(rng, 2, 48, 48), 2, 48, 48, 1.0))
    cases.append(Case("254/255 blocks", u8_saturated(O, rng, (36, 30, 40)), _camera(rng, 3, 50, 38), 3, 50, 38, 0.5))
    cases.append(Case("stand-in", O.volume_standin_u8((48, 40, 56), seed=5), _camera(rng, 0, 64, 48), 0, 64, 48, 1.0, half=True))
    cases.append(Case("fog", O.volume_fog_u8((40, 24, 56), seed=7, lo=20, span=12), _camera(rng, 1, 48, 48), 1, 48, 48, 0.5))
    # tiles: one that starts off screen, one inside, one that runs off the far corner
    cam = (0.9, 0.4, 0.8, (0.5, 0.5, 0.5), 64 / 48)
    cases.append(Case("tile at a negative origin", f16_edges(O, rng, (37, 29, 41)), cam, 0, 64, 48, 0.5, tile=(-9, -6, 40, 30), tags=("edge",)))
    cases.append(Case("tile inside", u8_speckle(O, rng, (29, 35, 30)), cam, 0, 64, 48, 1.0, tile=(13, 7, 31, 22), tags=("edge",)))
    cases.append(Case("tile past the corner", f16_nonfinite_ball(O, rng, (30, 30, 30)), cam, 0, 64, 48, 1.7, tile=(40, 30, 40, 40),
                      tags=("edge",)))
    return tuple(cases)


N_CASES = N_RANDOM + len(FIXED_DIMS) + 15


def cases(O):
    """The case list (deterministic: built once from SEED).  O: the oracle module (tests' `O` fixture)."""
    out = _cases(O)
    assert len(out) == N_CASES, len(out)
    return out
