"""The seeded fuzz cases of light-direction shadows under a first-hit isosurface (vk_set_shadows), shared by tests/test_shadow_fuzz_cpu.py
(the numpy reference against the C restatement) and tests/test_shadow_fuzz_gpu.py (the kernels against the C restatement).

In the manner of tests/iso_cases.py: volumes, cameras and lights come from tests/table_cases.py and tests/u16_cases.py, the kinds of
volume (u8, f16, u16), light, refinement depth, bias, strength and dt are dealt in cycles of coprime lengths and the draw fills in their
parameters; the named cases pin the edges -- dims from 1x1x1, tiles at a negative origin and inside the frame, a caster and a receiver,
a clip box that removes the caster, cut faces towards and away from the light, bias 0 and bias 1024, strength 0 and 1, axis-aligned
lights, a threshold above all data.  Every case is lit by a light that is not a headlight (shadows are ignored otherwise).  `mask`
marks the cases rendered with ambient 0, specular 0, diffuse 1, strength 1 and colour (1, 1, 1), where a shadowed pixel is exactly 0."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import table_cases as TC
import u16_cases as UC

SEED = 20261021
DTS = TC.DTS
N_RANDOM = 18
FIXED_DIMS = TC.FIXED_DIMS
REFINES = (4, 0, 16, 1)
LIGHTS = ("random", "+x", "random", "-x", "view")
BIASES = (2.0, 1.0, 0.5, 4.0, 2.0, 8.0, 1.5)
STRENGTHS = (0.7, 1.0, 0.25, 0.0, 0.9)
MASK_LIGHT = dict(ambient=0.0, diffuse=1.0, specular=0.0, shininess=32.0)


@dataclass
class Case:
    name: str
    vol: np.ndarray            # (nz, ny, nx) u8, f16 or uint16 (R16_UNORM)
    cam: tuple                 # arguments of oracle.camera_blob
    W: int
    H: int
    dt: float
    iso: float                 # threshold in sample values
    light: dict                # keyword arguments of Context.set_lighting; never a headlight
    shadows: tuple = (0.7, 2.0)  # (strength, bias)
    colour: tuple = (1.0, 1.0, 1.0)
    refine: int = 4
    box: tuple | None = None   # (lo3, hi3)
    tile: tuple | None = None
    half: bool = False
    mask: bool = False
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.vol.shape
        return nx, ny, nz

    @property
    def kind(self):
        return {np.dtype(np.uint8): "u8", np.dtype(np.float16): "f16", np.dtype(np.uint16): "u16"}[self.vol.dtype]

    def __repr__(self):
        return (f"ShadowCase({self.name}: dims={self.dims} {self.kind} {self.W}x{self.H} tile={self.tile} dt={self.dt} iso={self.iso} R={self.refine} "
                f"light={self.light['direction']} shadows={self.shadows} box={self.box} mask={self.mask})")


def two_balls(dims, centres=((0.28, 0.5, 0.5), (0.74, 0.5, 0.5)), radii=(0.16, 0.2), shell=0.12):
    """Two solid balls (255 inside, falling to 0 over `shell`) in empty space: with the light along the line through their centres one
    casts its shadow on the other."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    v = np.zeros(x.shape)
    for c, r in zip(centres, radii):
        d = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        v = np.maximum(v, np.clip((r + 0.5 * shell - d) / shell * 255.0, 0.0, 255.0))
    return v.round().astype(np.uint8)


def _mask_light(direction):
    return dict(direction=direction, **MASK_LIGHT)


def _volume(O, rng, kind, dims):
    """(volume, threshold in sample values)."""
    if kind == "u8 blobs":
        return TC.u8_blobs(O, rng, dims), float(rng.uniform(0.25, 0.5))
    if kind == "u8 standin":
        return TC.u8_standin(O, rng, dims), float(rng.uniform(0.2, 0.45))
    if kind == "f16 edges":
        return TC.f16_edges(O, rng, dims), float(rng.uniform(0.3, 0.8))
    if kind == "f16 finite":
        return TC.f16_finite(O, rng, dims), float(rng.uniform(0.3, 0.8))
    vk = kind.split()[1]
    return UC.VOLUMES[vk](O, rng, dims)[0], UC.ISO_OF[vk]


VKINDS = ("u8 blobs", "f16 edges", "u16 a", "u8 standin", "u16 b", "f16 finite", "u16 e")


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    cases = []
    for trial in range(N_RANDOM):
        dt = DTS[trial % len(DTS)]
        vkind = VKINDS[trial % len(VKINDS)]
        hi_dims = 14 if dt < 0.1 else 64
        dims = tuple(int(x) for x in rng.integers(5, hi_dims + 1, 3))
        W, H = int(rng.integers(24, 81)), int(rng.integers(24, 81))
        if dt < 0.1:
            W, H = min(W, 32), min(H, 32)
        cam = UC._iso_camera(rng, trial % 4, W, H) if trial % 3 else TC._camera(rng, trial % 4, W, H)
        vol, iso = _volume(O, rng, vkind, dims)
        mask = trial % 3 == 1
        lkind = LIGHTS[trial % len(LIGHTS)]
        light = TC._light(O, rng, lkind, cam)
        if mask:  # (a random direction: under an axis-aligned light flat data gives |N.L| = 0 on whole faces, which a mask case must not hold)
            lkind = "random"
            light = _mask_light(tuple(float(v) for v in rng.normal(size=3)))
        shadows = (1.0 if mask else STRENGTHS[trial % len(STRENGTHS)], BIASES[trial % len(BIASES)])
        colour = (1.0, 1.0, 1.0) if mask else tuple(float(v) for v in rng.uniform(0.0, 1.0, 3))
        cases.append(Case(f"r{trial:02d}", vol, cam, W, H, dt, iso, light, shadows, colour, REFINES[trial % len(REFINES)],
                          box=UC._box(rng) if trial % 5 == 2 else None, mask=mask, tags=(vkind, lkind)))
    # dims that straddle the packed layouts' cell and brick edges, from a single voxel up
    for j, dims in enumerate(FIXED_DIMS):
        vkind = ("u8 standin", "f16 edges", "u16 a", "u8 standin", "u16 e")[j]
        cam = TC._camera(rng, (0, 1, 0, 2, 0)[j], 40, 32)
        vol, iso = _volume(O, rng, vkind, dims)
        if vol.size == 1:
            vol[...] = 200
        light = TC._light(O, rng, ("random", "+x", "random", "view", "-x")[j], cam)
        cases.append(Case(f"dims{'x'.join(map(str, dims))}", vol, cam, 40, 32, (0.5, 1.0, 0.15, 3.5, 1.7)[j], (0.3, 0.2, iso, 0.4, iso)[j], light,
                          (0.7, (2.0, 1.0, 0.5, 1.0, 2.0)[j]), refine=(4, 16, 1, 0, 4)[j], tags=(vkind,)))
    side = (0.7, 0.2, 0.0, (0.5, 0.5, 0.5), 64 / 48)  # seen from the side: both balls in view, the light runs across the frame
    # a caster and a receiver: the light comes from +x, the ball at high x shadows the ball at low x; a mask case
    cases.append(Case("caster and receiver", two_balls((48, 40, 44)), side, 64, 48, 0.5, 0.5, _mask_light((1.0, 0.0, 0.0)), (1.0, 2.0), mask=True,
                      tags=("+x",)))
    # ... and under a clip box that removes the caster: the receiver's lit side comes out of the shadow
    cases.append(Case("caster clipped away", two_balls((48, 40, 44)), side, 64, 48, 0.5, 0.5, _mask_light((1.0, 0.0, 0.0)), (1.0, 2.0),
                      box=((0.0, 0.0, 0.0), (0.5, 1.0, 1.0)), mask=True, tags=("+x",)))
    # the same pair under a slanted light, shaded in full, in tiles: one at a negative origin, one inside the frame
    slanted = dict(direction=(1.0, 0.35, 0.2), ambient=0.2, diffuse=0.8, specular=0.5, shininess=16.0)
    cases.append(Case("tile at a negative origin", two_balls((37, 29, 41)), side, 64, 48, 0.5, 0.4, slanted, (0.7, 2.0), (0.9, 0.6, 0.3),
                      tile=(-9, -6, 48, 40)))
    cases.append(Case("tile inside", two_balls((33, 40, 29)), side, 56, 48, 1.0, 0.4, slanted, (0.7, 2.0), (0.2, 0.7, 0.9), tile=(8, 16, 32, 24)))
    # bias 0: the first shadow sample is the crossing itself; the surface lies inside the box, every hit is shadowed
    cases.append(Case("bias 0", two_balls((40, 36, 32)), side, 48, 40, 0.5, 0.5, _mask_light((0.4, 1.0, -0.3)), (1.0, 0.0), refine=16, mask=True))
    # bias 1024: ts0 lies beyond the box, no shadow ray has an iteration
    cases.append(Case("bias 1024", two_balls((40, 36, 32)), side, 48, 40, 0.5, 0.5, _mask_light((1.0, 0.0, 0.0)), (1.0, 1024.0), mask=True))
    # strength 0 (nothing changes) and strength 1 (only the ambient term is left), shaded in full
    full = dict(direction=(1.0, 0.2, 0.1), ambient=0.25, diffuse=0.9, specular=0.6, shininess=24.0)
    cases.append(Case("strength 0", two_balls((36, 30, 34)), side, 48, 40, 0.5, 0.5, full, (0.0, 2.0), (0.8, 0.7, 0.6)))
    cases.append(Case("strength 1", two_balls((36, 30, 34)), side, 48, 40, 0.5, 0.5, full, (1.0, 2.0), (0.8, 0.7, 0.6)))
    # cut faces: the threshold lies below all data, every ray hits in its first iteration on a face of the box (or of a clip box); the
    # faces towards the light are lit (their shadow rays leave the box at once: no iteration, or tb0 > tb1 where the hit position rounded
    # outside under an axis-aligned light), the others are shadowed by the material behind them
    corner = (1.6, 0.6, 0.8, (0.5, 0.5, 0.5), 48 / 40)
    cases.append(Case("cut faces, light +x", O.volume_standin_u8((40, 33, 27), seed=11), corner, 48, 40, 0.5, -0.5, _mask_light((1.0, 0.0, 0.0)), (1.0, 2.0),
                      refine=16, tags=("+x",)))  # (no mask case: the face towards the light has a clamped x-gradient, |N.L| = 0 all over it)
    cases.append(Case("cut faces, light -x, clip box", O.volume_standin_u8((40, 33, 27), seed=11), corner, 48, 40, 0.5, -0.5, _mask_light((-1.0, 0.0, 0.0)),
                      (1.0, 2.0), box=((0.2, 0.1, 0.15), (0.8, 0.9, 0.7)), mask=True, tags=("-x",)))
    cases.append(Case("cut faces, f16, slanted light", TC.f16_finite(O, rng, (21, 30, 18)), corner, 48, 40, 0.15, -70000.0,
                      dict(direction=(0.3, 1.0, 0.5), ambient=0.1, diffuse=1.0, specular=0.3, shininess=8.0), (0.6, 2.0), (0.5, 0.5, 0.5)))
    # the threshold above all data: no hits, no shadow rays
    cases.append(Case("iso above all data", O.volume_standin_u8((33, 17, 65), seed=9), TC._camera(rng, 0, 48, 40), 48, 40, 0.5, 2.0,
                      TC._light(O, rng, "random", corner), (0.7, 2.0)))
    # half-float output: PACKED_PAIRS (u8), PACKED f16 and u16 at dt 0.5
    cam = UC._iso_camera(rng, 0, 48, 36)
    cases.append(Case("rgba16f u8", two_balls((36, 44, 28)), cam, 48, 36, 0.5, 0.3, slanted, (0.7, 2.0), (0.9, 0.8, 0.2), half=True))
    cases.append(Case("rgba16f f16", TC.f16_edges(O, rng, (30, 26, 35)), cam, 48, 36, 0.5, 0.5, TC._light(O, rng, "random", cam), (0.7, 1.0), (0.1, 0.6, 0.9),
                      half=True))
    cases.append(Case("rgba16f u16", UC.vol_a(O, rng, (29, 33, 31))[0], cam, 48, 36, 0.5, UC.ISO_OF["a"], _mask_light((0.5, 0.6, 0.7)), (1.0, 2.0), mask=True,
                      half=True))
    return tuple(cases)


N_CASES = N_RANDOM + len(FIXED_DIMS) + 15


def cases(O):
    """The case list (deterministic: built once from SEED).  O: the oracle module (tests' `O` fixture)."""
    out = _cases(O)
    assert len(out) == N_CASES, len(out)
    return out
