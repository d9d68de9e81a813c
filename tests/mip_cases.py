"""The seeded fuzz cases of the maximum-intensity projection (vk_set_projection(VK_PROJ_MAX)), shared by tests/test_mip_fuzz_cpu.py (the
numpy reference against the C restatement) and tests/test_mip_fuzz_gpu.py (the kernels against the C restatement).

In the manner of tests/table_cases.py, whose cameras, volumes and table generators are reused: the kinds of camera, volume, table, window
and dt are dealt in cycles of coprime lengths, the draw fills in their parameters; the named cases pin the edges -- dims from 1x1x1, a tile
at a negative origin, the grey ramp that stands for "no table", tables with -0 entries and colours at +-VK_TF_MAX_COLOUR, u8 data at 0 / 255
and around the window's ends, windows under which every cell or no cell is empty, half-float output."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import table_cases as TC

SEED = 20261017
DTS = TC.DTS
N_RANDOM = 42
FIXED_DIMS = TC.FIXED_DIMS


@dataclass
class Case:
    name: str
    vol: np.ndarray            # (nz, ny, nx) u8 or f16
    cam: tuple                 # arguments of oracle.camera_blob
    W: int
    H: int
    dt: float
    table: np.ndarray | None   # (n, 4) f32, or None: no table is set (the implicit grey ramp over [0, 1])
    domain: tuple = (0.0, 1.0)
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

    @property
    def n(self):
        return 2 if self.table is None else self.table.shape[0]

    def __repr__(self):
        return (f"MipCase({self.name}: dims={self.dims} {'f16' if self.f16 else 'u8'} {self.W}x{self.H} tile={self.tile} dt={self.dt} "
                f"n={'none' if self.table is None else self.n} window={self.domain})")


# ---- tables (the alpha column is not read under MAX) ----

def signed_zero_table(rng, n):
    """Entries that are -0 and +0 in every channel, the first entry -0: a U of -0 would show in the sign of the lerp."""
    t = TC.random_table(rng, n)
    t[0, :3] = -0.0
    t[-1, :3] = 0.0
    if n >= 3:
        t[int(rng.integers(1, n - 1)), :3] = -0.0
    return t


TABLES = {"random": TC.random_table, "big": TC.big_table, "signed zero": signed_zero_table}


# ---- windows ----

def _window(kind, f16):
    if kind == "unit":
        return (0.0, 1.0)
    if kind == "inside":  # inside the data's range: both ends are reached
        return (0.3, 0.6)
    if kind == "narrow":  # much narrower than the data
        return (0.3, 0.30001)
    if kind == "wide":
        return (-2.5, 7.25)
    if kind == "below":  # the window lies below the data: u = n - 1 at the first finite sample
        return (-9.0, -5.0) if f16 else (-3.0, -1.0)
    return (70000.0, 80000.0) if f16 else (2.0, 5.0)  # "above": u = 0 everywhere


WINDOWS = ("unit", "inside", "narrow", "wide", "below", "above", "inside")


# ---- volumes ----

def u8_window_ends(O, rng, dims):
    """u8 data at 0, 255 and around the ends of the window (0.3, 0.6): 76.5 and 153 on the 0..255 scale."""
    return rng.choice(np.array([0, 0, 0, 255, 75, 76, 77, 78, 152, 153, 154], np.uint8), dims[::-1]).astype(np.uint8)


VOLUMES = dict(TC.VOLUMES)
VOLUMES["u8 window ends"] = u8_window_ends


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    cases = []
    vkinds, tkinds, ns = tuple(VOLUMES), tuple(TABLES), (2, 3, 17, 256)
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
        wkind = WINDOWS[trial % len(WINDOWS)]
        tkind = tkinds[trial % len(tkinds)]
        if trial % 11 == 5:  # no table: the grey ramp over [0, 1]
            table, window, tkind = None, (0.0, 1.0), "none"
        else:
            table, window = TABLES[tkind](rng, ns[trial % len(ns)]), _window(wkind, vol.dtype == np.float16)
        cases.append(Case(f"r{trial:02d}", vol, cam, W, H, dt, table, window, tags=(vkind, tkind, wkind)))
    # dims that straddle the packed layouts' cell and brick edges, from a single voxel up
    for j, dims in enumerate(FIXED_DIMS):
        f16 = j % 2 == 1
        cam = TC._camera(rng, j % 4, 40, 32)
        vol = TC.f16_edges(O, rng, dims) if f16 else TC.u8_standin(O, rng, dims)
        table = (TC.random_table(rng, 17), None, signed_zero_table(rng, 3), TC.random_table(rng, 2), TC.big_table(rng, 256))[j]
        cases.append(Case(f"dims{'x'.join(map(str, dims))}", vol, cam, 40, 32, (0.5, 1.0, 0.15, 3.5, 1.7)[j], table,
                          (0.0, 1.0) if not f16 or table is None else (-0.5, 1.5)))
    # short rays over noise: some ray's maximum comes from its last iteration
    cases.append(Case("short rays over noise", rng.integers(0, 256, (5, 6, 7)).astype(np.uint8), TC._camera(rng, 0, 48, 40), 48, 40, 1.7,
                      TC.random_table(rng, 17), (0.0, 1.0)))
    # a tile that starts off screen, at a negative origin
    cases.append(Case("tile at a negative origin", TC.u8_blobs(O, rng, (37, 29, 41)), (0.9, 0.4, 0.8, (0.5, 0.5, 0.5), 64 / 48), 64, 48, 0.5,
                      TC.random_table(rng, 256), (0.1, 0.8), tile=(-9, -6, 40, 30)))
    cases.append(Case("tile inside, no table", TC.u8_standin(O, rng, (33, 40, 29)), TC._camera(rng, 0, 56, 48), 56, 48, 1.0, None, tile=(8, 16, 24, 16)))
    # every cell empty: the data lies below the window (u = 0 everywhere); the walks are clamped to the trip budget
    cases.append(Case("every cell empty", O.volume_standin_u8((33, 17, 65), seed=9), TC._camera(rng, 0, 48, 40), 48, 40, 0.5,
                      signed_zero_table(rng, 17), (2.0, 5.0), empty=1.0))
    cases.append(Case("every cell empty, f16", TC.f16_finite(O, rng, (21, 30, 18)), TC._camera(rng, 1, 48, 40), 48, 40, 0.15,
                      TC.random_table(rng, 256), (70000.0, 80000.0), empty=1.0))
    cases.append(Case("every cell empty, no table", np.zeros((19, 23, 30), np.uint8), TC._camera(rng, 0, 40, 40), 40, 40, 0.5, None, empty=1.0))
    # no cell empty: the data lies above the window (u = n - 1 at every sample)
    cases.append(Case("no cell empty", O.volume_standin_u8((40, 33, 27), seed=11), TC._camera(rng, 1, 48, 40), 48, 40, 0.5,
                      TC.random_table(rng, 256), (-3.0, -1.0), empty=0.0))
    # no cell empty and no ray saturates: u8 data of at least 1 under the grey ramp (u > 0 in every cell, u < 1 below 255)
    cases.append(Case("no cell empty, no table", rng.integers(1, 255, (26, 31, 22)).astype(np.uint8), TC._camera(rng, 0, 48, 40), 48, 40, 0.5, None,
                      empty=0.0))
    # half-float output: one PACKED_PAIRS (u8) and one PACKED f16 case at dt 0.5
    cam = TC._camera(rng, 0, 48, 36)
    cases.append(Case("rgba16f u8", TC.u8_standin(O, rng, (36, 44, 28)), cam, 48, 36, 0.5, TC.random_table(rng, 256), (0.05, 0.9), half=True))
    cases.append(Case("rgba16f f16", TC.f16_edges(O, rng, (30, 26, 35)), cam, 48, 36, 0.5, TC.random_table(rng, 17), (-0.5, 1.5), half=True))
    # colours at +-VK_TF_MAX_COLOUR over f16 data with every special value
    cases.append(Case("colours at the bound, f16", TC.f16_edges(O, rng, (27, 19, 33)), TC._camera(rng, 0, 40, 40), 40, 40, 1.0, TC.big_table(rng, 17),
                      (-0.5, 1.5)))
    return tuple(cases)


N_CASES = N_RANDOM + len(FIXED_DIMS) + 11


def cases(O):
    """The case list (deterministic: built once from SEED).  O: the oracle module (tests' `O` fixture)."""
    out = _cases(O)
    assert len(out) == N_CASES, len(out)
    return out
