"""The seeded fuzz cases of first-hit isosurface rendering (vk_set_isosurface), shared by tests/test_iso_fuzz_cpu.py (the numpy reference
against the C restatement) and tests/test_iso_fuzz_gpu.py (the kernels against the C restatement).

In the manner of tests/mip_cases.py: the cameras, volumes and lights of tests/table_cases.py are reused, and the kinds of camera, volume,
threshold, refinement depth, light and dt are dealt in cycles of coprime lengths, the draw fills in their parameters; the named cases pin
the edges -- dims from 1x1x1, a tile at a negative origin and one inside the frame, a hit by equality on 255 plateaus, thresholds below
and above all data, the lighting coefficients at their bounds, half-float output."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import table_cases as TC

SEED = 20261019
DTS = TC.DTS
N_RANDOM = 45
FIXED_DIMS = TC.FIXED_DIMS
REFINES = (0, 1, 4, 16)
LIGHTS = ("none", "headlight", "+x", "random", "view", "none", "-x")  # none / headlight / fixed / random


@dataclass
class Case:
    name: str
    vol: np.ndarray            # (nz, ny, nx) u8 or f16
    cam: tuple                 # arguments of oracle.camera_blob
    W: int
    H: int
    dt: float
    iso: float                 # threshold in sample values
    colour: tuple = (1.0, 1.0, 1.0)
    refine: int = 4
    light: dict | None = None  # keyword arguments of Context.set_lighting
    tile: tuple | None = None
    empty: float | None = None  # the packed layouts' empty fraction this case must report
    half: bool = False
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.vol.shape
        return nx, ny, nz

    @property
    def f16(self):
        return self.vol.dtype == np.float16

    def __repr__(self):
        lt = None if self.light is None else self.light["direction"]
        return (f"IsoCase({self.name}: dims={self.dims} {'f16' if self.f16 else 'u8'} {self.W}x{self.H} tile={self.tile} dt={self.dt} "
                f"iso={self.iso} R={self.refine} light={lt})")


# ---- thresholds ----

def _iso(rng, kind, f16):
    """A threshold in sample values: inside the data's range (u8: normalised; f16: the blobs reach ~1.6)."""
    if kind == "low":
        return float(rng.uniform(0.08, 0.2))
    if kind == "mid":
        return float(rng.uniform(0.3, 0.55))
    if kind == "high":
        return float(rng.uniform(0.7, 1.2 if f16 else 0.95))
    if kind == "grid":  # on a data value: u8 k / 255 (the product with 255.0f need not be k); f16 a value the data holds
        return float(np.float16(rng.uniform(0.2, 0.9))) if f16 else int(rng.integers(30, 250)) / 255.0
    return 0.0  # "zero": every sample >= +-0 hits; negative f16 data does not


ISOS = ("low", "mid", "high", "grid", "mid", "zero", "low", "mid")


def _colour(rng, j):
    if j % 5 == 3:
        return (float(TC.TF_MAX_COLOUR), -float(TC.TF_MAX_COLOUR), -0.0)
    return tuple(float(v) for v in rng.uniform(0.0, 1.0, 3))


def u8_plateaus(O, rng, dims):
    """Plateaus of 255 in air with ramps between them: a ray reaches 255.0 exactly inside a plateau."""
    vol = TC._blobs(rng, dims, 0.0, (400.0, 900.0), count=3)
    return np.clip(vol, 0, 255).astype(np.uint8)


VOLUMES = dict(TC.VOLUMES)


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    cases = []
    vkinds = tuple(VOLUMES)
    for trial in range(N_RANDOM):
        dt = DTS[trial % len(DTS)]
        vkind = vkinds[trial % len(vkinds)]
        hi_dims = 16 if dt < 0.1 else 64
        dims = tuple(int(x) for x in rng.integers(5, hi_dims + 1, 3))
        W, H = int(rng.integers(24, 81)), int(rng.integers(24, 81))
        if dt < 0.1:
            W, H = min(W, 40), min(H, 40)
        cam = TC._camera(rng, trial % 4, W, H)
        vol = VOLUMES[vkind](O, rng, dims)
        ikind = ISOS[trial % len(ISOS)]
        light = TC._light(O, rng, LIGHTS[trial % len(LIGHTS)], cam)
        cases.append(Case(f"r{trial:02d}", vol, cam, W, H, dt, _iso(rng, ikind, vol.dtype == np.float16), _colour(rng, trial),
                          REFINES[trial % len(REFINES)], light, tags=(vkind, ikind, LIGHTS[trial % len(LIGHTS)])))
    # dims that straddle the packed layouts' cell and brick edges, from a single voxel up
    for j, dims in enumerate(FIXED_DIMS):
        f16 = j % 2 == 1
        cam = TC._camera(rng, j % 4, 40, 32)
        vol = TC.f16_edges(O, rng, dims) if f16 else TC.u8_standin(O, rng, dims)
        light = TC._light(O, rng, ("headlight", "random", "none", "view", "+x")[j], cam)
        cases.append(Case(f"dims{'x'.join(map(str, dims))}", vol, cam, 40, 32, (0.5, 1.0, 0.15, 3.5, 1.7)[j], (0.3, 0.2, 0.5, 0.4, 0.25)[j],
                          _colour(rng, j), (4, 16, 1, 0, 4)[j], light))
    # a tile that starts off screen, at a negative origin; a tile inside the frame
    cases.append(Case("tile at a negative origin", TC.u8_blobs(O, rng, (37, 29, 41)), (0.9, 0.4, 0.8, (0.5, 0.5, 0.5), 64 / 48), 64, 48, 0.5, 0.35,
                      (0.9, 0.6, 0.3), 4, dict(direction="headlight", ambient=0.2, diffuse=0.8, specular=0.5, shininess=16.0), tile=(-9, -6, 40, 30)))
    cases.append(Case("tile inside", TC.u8_standin(O, rng, (33, 40, 29)), TC._camera(rng, 0, 56, 48), 56, 48, 1.0, 0.3, (0.2, 0.7, 0.9), 4, None,
                      tile=(8, 16, 24, 16)))
    # a hit by equality: iso = 1.0 over u8 data with plateaus of 255 gives iso_k == 255.0f exactly
    cases.append(Case("hit by equality on 255 plateaus", u8_plateaus(O, rng, (30, 34, 27)), TC._camera(rng, 0, 48, 40), 48, 40, 0.5, 1.0, (1.0, 0.5, 0.25), 4,
                      TC._light(O, rng, "random", (1.0, 0.3, 0.4, (0.5, 0.5, 0.5), 1.2))))
    # the threshold below all data: no cell is empty, every ray hits in its first iteration (and is not refined)
    cam = TC._camera(rng, 0, 48, 40)
    cases.append(Case("iso below all data", O.volume_standin_u8((40, 33, 27), seed=11), cam, 48, 40, 0.5, -0.5, (0.3, 0.9, 0.4), 16,
                      TC._light(O, rng, "view", cam), empty=0.0))
    cases.append(Case("iso below all data, f16", TC.f16_finite(O, rng, (21, 30, 18)), TC._camera(rng, 1, 48, 40), 48, 40, 0.15, -70000.0,
                      (0.5, 0.5, 0.5), 4, None, empty=0.0))
    # the threshold above all data: every cell is empty, the frame is all background; the walks are clamped to the trip budget
    cam = TC._camera(rng, 0, 48, 40)
    cases.append(Case("iso above all data", O.volume_standin_u8((33, 17, 65), seed=9), cam, 48, 40, 0.5, 2.0, (1.0, 1.0, 1.0), 4,
                      TC._light(O, rng, "headlight", cam), empty=1.0))
    cases.append(Case("iso above all data, f16", TC.f16_finite(O, rng, (21, 30, 18)), TC._camera(rng, 1, 48, 40), 48, 40, 0.15, 70000.0,
                      (1.0, 1.0, 1.0), 1, None, empty=1.0))
    # every coefficient at 16, with the flattest and the sharpest highlight
    cam = TC._camera(rng, 0, 40, 40)
    cases.append(Case("lit at the bounds, shininess 1", TC.u8_blobs(O, rng, (31, 42, 23)), cam, 40, 40, 0.5, 0.4, (0.8, 0.7, 0.6), 4,
                      dict(direction="headlight", ambient=16.0, diffuse=16.0, specular=16.0, shininess=1.0)))
    cases.append(Case("lit at the bounds, shininess 1024", TC.u8_blobs(O, rng, (31, 42, 23)), cam, 40, 40, 0.5, 0.4, (0.8, 0.7, 0.6), 16,
                      dict(direction=(0.3, -1.0, 0.2), ambient=16.0, diffuse=16.0, specular=16.0, shininess=1024.0)))
    # half-float output: one PACKED_PAIRS (u8) and one PACKED f16 case at dt 0.5
    cam = TC._camera(rng, 0, 48, 36)
    cases.append(Case("rgba16f u8", TC.u8_standin(O, rng, (36, 44, 28)), cam, 48, 36, 0.5, 0.3, (0.9, 0.8, 0.2), 4, TC._light(O, rng, "headlight", cam),
                      half=True))
    cases.append(Case("rgba16f f16", TC.f16_edges(O, rng, (30, 26, 35)), cam, 48, 36, 0.5, 0.5, (0.1, 0.6, 0.9), 4, None, half=True))
    # coarse steps through a smooth ball: the crossing lies anywhere within the step, deep bisection
    from lit_helpers import sphere_u8
    cases.append(Case("coarse steps through a ball", sphere_u8(24, 20, 28), (1.4, 0.3, 0.7, (0.5, 0.5, 0.5), 1.0), 48, 48, 3.5, 0.5, (0.8, 0.8, 0.8), 16,
                      dict(direction=(1.0, 1.0, 0.5), ambient=0.2, diffuse=0.8, specular=0.4, shininess=24.0)))
    # finite thresholds whose iso_k overflows on R8 (iso * 255.0f): -inf is met by every sample, a ray with no iteration stays background;
    # +inf is met by none
    cam = TC._camera(rng, 0, 40, 32)
    cases.append(Case("iso_k overflows to -inf", TC.u8_standin(O, rng, (19, 23, 17)), cam, 40, 32, 0.5, -3.0e38, (0.4, 0.5, 0.6), 4,
                      TC._light(O, rng, "headlight", cam), empty=0.0))
    cases.append(Case("iso_k overflows to +inf", TC.u8_standin(O, rng, (19, 23, 17)), cam, 40, 32, 1.0, 3.0e38, (0.4, 0.5, 0.6), 4, None, empty=1.0))
    return tuple(cases)


N_CASES = N_RANDOM + len(FIXED_DIMS) + 14


def cases(O):
    """The case list (deterministic: built once from SEED).  O: the oracle module (tests' `O` fixture)."""
    out = _cases(O)
    assert len(out) == N_CASES, len(out)
    return out
