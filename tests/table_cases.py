"""The seeded fuzz cases of the table march and the lit table march, shared by tests/test_table_fuzz_cpu.py (the numpy reference against
the C restatements) and tests/test_table_fuzz_gpu.py (the kernels against the C restatements), so that both walk the same list.

Each case fixes the volume (u8 or f16), the camera (orbit, eye inside, axis-aligned, grazing a face), the image and an optional tile, dt_scale,
the table and its domain, and the lighting (None: the unlit table).  Coverage does not hang on the draw: the kinds of camera, volume, table,
domain, dt and light are dealt in cycles of coprime lengths, the draw only fills in their parameters; the named cases pin the edges
(tiny and brick-straddling dims, a tile that starts off screen, domains under which every cell or no cell is empty, half-float output)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

SEED = 20261016
DTS = (0.013, 0.15, 0.5, 1.0, 1.7, 3.5)
N_RANDOM = 48
FIXED_DIMS = ((1, 1, 1), (2, 3, 5), (4, 4, 4), (5, 4, 9), (33, 17, 65))
TF_MAX_COLOUR = 1e30  # VK_TF_MAX_COLOUR
# f16 NaNs written as bit patterns: quiet, signalling, signalling with the sign set
F16_NAN_BITS = (0x7E00, 0x7C01, 0xFC01)


@dataclass
class Case:
    name: str
    vol: np.ndarray            # (nz, ny, nx) u8 or f16
    cam: tuple                 # arguments of oracle.camera_blob: zoom, pitch, yaw, target, aspect
    W: int
    H: int
    dt: float
    table: np.ndarray          # (n, 4) f32
    domain: tuple
    light: dict | None = None  # keyword arguments of Context.set_lighting
    tile: tuple | None = None  # (tx, ty, tw, th), any origin
    empty: float | None = None  # the packed layouts' empty fraction this case must report
    half: bool = False         # also render RGBA16F output
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.vol.shape
        return nx, ny, nz

    @property
    def f16(self):
        return self.vol.dtype == np.float16

    @property
    def big(self):
        """A table with colours near VK_TF_MAX_COLOUR: colour is compared relative to max(1, |ref|)."""
        return float(np.abs(self.table[:, :3]).max()) > 1e6

    def __repr__(self):
        lt = None if self.light is None else self.light["direction"]
        return (f"Case({self.name}: dims={self.dims} {'f16' if self.f16 else 'u8'} {self.W}x{self.H} tile={self.tile} dt={self.dt} "
                f"n={self.table.shape[0]} domain={self.domain} light={lt})")


# ---- cameras (the four kinds of tests/test_parity_gpu.py::test_skip_fuzz_cameras_dims_dt) ----

def _camera(rng, kind, W, H):
    if kind == 0:    # ordinary orbit
        return (float(rng.uniform(0.7, 2.5)), float(rng.uniform(-1.4, 1.4)), float(rng.uniform(0, 6.28)), (0.5, 0.5, 0.5), W / H)
    if kind == 1:    # eye inside the volume
        return (float(rng.uniform(0.05, 0.4)), float(rng.uniform(-1.0, 1.0)), float(rng.uniform(0, 6.28)),
                tuple(float(x) for x in rng.uniform(0.3, 0.7, 3)), W / H)
    if kind == 2:    # axis-aligned views: direction components that are exactly zero on the centre rays
        return (1.5, 0.0, float(rng.integers(0, 4)) * 1.5707963, (0.5, 0.5, 0.5), 1.0)
    return (1.2, float(rng.uniform(-0.05, 0.05)), float(rng.uniform(0, 6.28)), (0.5, float(rng.choice([0.02, 0.98])), 0.5), W / H)  # grazing a face


def view_axis(O, cam):
    """The direction from the camera's target to its eye (the eye: the first three floats of the camera blob)."""
    eye = np.frombuffer(O.camera_blob(*cam), np.float32)[:3].astype(np.float64)
    return tuple(float(v) for v in eye - np.array(cam[3]))


# ---- tables ----

def random_table(rng, n):
    """Random RGBA with a run of alpha exactly +0 and one of -0.0, and entries of alpha 1 (the early-out); mostly faint, so that rays run long
    and half the time the low values are clear (the air of the volumes: cells to skip)."""
    t = np.empty((n, 4), np.float32)
    t[:, :3] = rng.uniform(0.0, 1.0, (n, 3))
    t[:, 3] = rng.uniform(0.0, 1.0, n) ** 3 * 0.4
    if n >= 3 and rng.random() < 0.5:
        t[:max(1, n // 8), 3] = 0.0
    if n >= 3:
        a = int(rng.integers(0, n - 1))
        t[a:a + max(1, n // 5), 3] = 0.0
        b = int(rng.integers(0, n - 1))
        t[b:b + max(1, n // 6), 3] = -0.0
        t[int(rng.integers(0, n)), 3] = 1.0
    else:
        t[int(rng.integers(0, 2)), 3] = 0.0
    return t


def inverted_table(rng, n):
    """Low values opaque, high values clear: under it the skip maps mark dense material empty and air not."""
    x = np.arange(n) / max(n - 1, 1)
    t = np.empty((n, 4), np.float32)
    t[:, :3] = np.stack([0.3 + 0.6 * x, np.full(n, 0.5), 1.0 - 0.8 * x], axis=1)
    t[:, 3] = np.where(x <= 0.5, rng.uniform(0.05, 0.3) * (1.0 - x), 0.0)
    t[-1, 3] = 0.0
    return t


def big_table(rng, n):
    """Colours up to +-VK_TF_MAX_COLOUR and negative colours (each channel keeps one sign: no cancellation between entries)."""
    t = random_table(rng, n)
    t[:, 0] = TF_MAX_COLOUR * rng.uniform(0.1, 1.0, n)
    t[:, 1] = -TF_MAX_COLOUR * rng.uniform(0.1, 1.0, n)
    t[:, 2] = -rng.uniform(0.0, 2.0, n)
    t[int(rng.integers(0, n)), 0] = TF_MAX_COLOUR
    t[int(rng.integers(0, n)), 1] = -TF_MAX_COLOUR
    return t


TABLES = {"random": random_table, "inverted": inverted_table, "big": big_table}


# ---- volumes ----

def _grid(dims):
    nx, ny, nz = dims
    return np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")


def _blobs(rng, dims, air, dense, count=4):
    z, y, x = _grid(dims)
    vol = np.full(x.shape, air, np.float64)
    for _ in range(count):
        c = rng.uniform(0.15, 0.85, 3) * np.array(dims)
        rad = rng.uniform(1.0, max(1.5, 0.35 * min(dims)))
        d2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
        vol = np.where(d2 < rad * rad, np.maximum(vol, rng.uniform(*dense) * (1.0 - np.sqrt(d2) / (1.5 * rad))), vol)
    return vol


def u8_standin(O, rng, dims):
    if min(dims) >= 17:
        return O.volume_standin_u8(dims, seed=int(rng.integers(1, 1 << 30)))
    return rng.integers(0, 256, dims[::-1]).astype(np.uint8)


def u8_blobs(O, rng, dims):
    """Blobs in air: air 0..20, blobs up to 255."""
    vol = _blobs(rng, dims, 0.0, (120.0, 255.0)) + rng.integers(0, 21, dims[::-1])
    return np.clip(vol, 0, 255).astype(np.uint8)


def u8_constant(O, rng, dims):
    """One value everywhere: every gradient is zero (the shade's no-gradient branch)."""
    return np.full(dims[::-1], int(rng.integers(0, 256)), np.uint8)


def f16_edges(O, rng, dims, hi=1.0, nonfinite=True):
    """f16 blobs in air with negative values, values beyond `hi`, +-0, subnormals and (nonfinite) +-inf and NaNs as bit patterns."""
    vol = _blobs(rng, dims, -0.05, (0.2, 1.6 * hi)) + rng.uniform(-0.1, 0.05, dims[::-1])
    bits = vol.astype(np.float16).view(np.uint16).copy()
    specials = [-3.0, -0.6, 3.5 * hi, 60000.0, 0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -17, 6.1e-5]
    sb = np.array(specials, np.float16).view(np.uint16)
    if nonfinite:
        sb = np.concatenate([sb, np.array([np.inf, -np.inf], np.float16).view(np.uint16), np.array(F16_NAN_BITS, np.uint16)])
    m = rng.random(bits.shape) < (0.03 if min(dims) > 2 else 0.3)
    bits[m] = rng.choice(sb, int(m.sum()))
    if nonfinite and bits.size >= 3:  # each NaN pattern at least once
        where = rng.choice(bits.size, 3, replace=False)
        bits.flat[where] = F16_NAN_BITS
    return bits.view(np.float16)


def f16_finite(O, rng, dims):
    return f16_edges(O, rng, dims, nonfinite=False)


VOLUMES = {"u8 standin": u8_standin, "u8 blobs": u8_blobs, "f16 edges": f16_edges, "u8 constant": u8_constant, "f16 finite": f16_finite}


# ---- domains ----

def _domain(kind, f16):
    """(lo, hi): normalised values for u8 volumes (the data lies in [0, 1]), values for f16 (the finite data lies in about [-3, 60000])."""
    if kind == "unit":
        return (0.0, 1.0)
    if kind == "narrow":
        return (0.3, 0.30001)
    if kind == "wide":
        return (-2.5, 7.25)
    if kind == "below":  # the domain lies below the data: u = n - 1 (all of it, for u8)
        return (-9.0, -5.0) if f16 else (-3.0, -1.0)
    return (70000.0, 80000.0) if f16 else (2.0, 5.0)  # "above": u = 0


DOMAINS = ("unit", "narrow", "wide", "below", "above", "unit", "wide")


# ---- lights ----

def _light(O, rng, kind, cam):
    if kind == "none":
        return None
    bounds = int(rng.integers(0, 3)) == 0
    if bounds:  # the parameters at their bounds
        ka, kd, ks = (float(rng.choice([0.0, 16.0])) for _ in range(3))
        n = float(rng.choice([1.0, 1024.0]))
    else:
        ka, kd, ks, n = float(rng.uniform(0, 1)), float(rng.uniform(0, 1.5)), float(rng.uniform(0, 1)), float(rng.uniform(1, 128))
    d = {"headlight": "headlight", "+x": (1.0, 0.0, 0.0), "-x": (-1.0, 0.0, 0.0), "view": view_axis(O, cam),
         "random": tuple(float(v) for v in rng.normal(size=3))}[kind]
    return dict(direction=d, ambient=ka, diffuse=kd, specular=ks, shininess=n)


LIGHTS = ("none", "headlight", "+x", "-x", "view", "random", "none", "headlight")


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    cases = []
    vkinds, tkinds, ns = tuple(VOLUMES), tuple(TABLES), (2, 3, 17, 256)
    for trial in range(N_RANDOM):
        dt = DTS[trial % len(DTS)]
        vkind = vkinds[trial % len(vkinds)]
        hi_dims = 16 if dt < 0.1 else 72  # (the smallest step: ~2000 iterations per ray over 16 cells)
        dims = tuple(int(x) for x in rng.integers(5, hi_dims + 1, 3))
        W, H = int(rng.integers(24, 97)), int(rng.integers(24, 97))
        if dt < 0.1:
            W, H = min(W, 48), min(H, 48)
        cam = _camera(rng, trial % 4, W, H)
        n = ns[trial % len(ns)]
        tkind = tkinds[trial % len(tkinds)]
        vol = VOLUMES[vkind](O, rng, dims)
        table = TABLES[tkind](rng, n)
        dkind = DOMAINS[trial % len(DOMAINS)]
        domain = _domain(dkind, vol.dtype == np.float16)
        if dkind in ("below", "above") and (trial // len(DOMAINS)) % 2 == 0:  # every other time, the entries the data reads are not clear
            end = slice(n - 2, n) if dkind == "below" else slice(0, 2)
            table[end, 3] = rng.uniform(0.05, 0.5, 2)
        light = _light(O, rng, LIGHTS[trial % len(LIGHTS)], cam)
        cases.append(Case(f"r{trial:02d}", vol, cam, W, H, dt, table, domain, light, tags=(vkind, tkind, dkind)))
    # dims that straddle the packed layouts' cell (4) and brick edges, and volumes that end partway through a brick
    for j, dims in enumerate(FIXED_DIMS):
        f16 = j % 2 == 1
        W, H = 40, 32
        cam = _camera(rng, j % 4, W, H)
        vol = f16_edges(O, rng, dims) if f16 else u8_standin(O, rng, dims)
        table = random_table(rng, (17, 256, 3, 2, 256)[j])
        light = _light(O, rng, ("headlight", "random", "none", "view", "+x")[j], cam)
        cases.append(Case(f"dims{'x'.join(map(str, dims))}", vol, cam, W, H, (0.5, 1.0, 0.15, 0.5, 1.7)[j], table,
                          (0.0, 1.0) if not f16 else (-0.5, 1.5), light))
    # a tile that starts off screen, at a negative origin
    cam = _camera(rng, 0, 64, 48)
    cases.append(Case("tile at a negative origin", u8_blobs(O, rng, (37, 29, 41)), (0.9, 0.4, 0.8, (0.5, 0.5, 0.5), 64 / 48), 64, 48, 0.5,
                      random_table(rng, 256), (0.0, 1.0), dict(direction="headlight", ambient=0.2, diffuse=0.8, specular=0.5, shininess=16.0),
                      tile=(-9, -6, 40, 30)))
    # every cell empty: the data lies below the domain (u = 0) and entries 0..2 have alpha 0; the walks are clamped to the trip budget
    t = random_table(rng, 17)
    t[:3, 3] = (0.0, -0.0, 0.0)
    cam = _camera(rng, 0, 48, 40)
    cases.append(Case("every cell empty", O.volume_standin_u8((33, 17, 65), seed=9), cam, 48, 40, 0.5, t, (2.0, 5.0), None, empty=1.0))
    cam = _camera(rng, 1, 48, 40)
    cases.append(Case("every cell empty, lit", f16_finite(O, rng, (21, 30, 18)), cam, 48, 40, 0.15, t, (70000.0, 80000.0),
                      _light(O, rng, "random", cam), empty=1.0))
    # no cell empty: the data lies above the domain (u = n - 1) and the last entry is opaque
    t = inverted_table(rng, 256)
    t[-1, 3] = 0.4
    cases.append(Case("no cell empty", O.volume_standin_u8((40, 33, 27), seed=11), cam, 48, 40, 0.5, t, (-3.0, -1.0), _light(O, rng, "view", cam),
                      empty=0.0))
    # the inverted table on a volume of air and dense material: the skip maps mark the material empty
    cam = _camera(rng, 0, 56, 44)
    cases.append(Case("inverted table, dense material empty", u8_blobs(O, rng, (45, 38, 52)), cam, 56, 44, 0.5, inverted_table(rng, 256),
                      (0.0, 1.0), _light(O, rng, "-x", cam)))
    # half-float output: one PACKED_PAIRS (u8) and one PACKED f16 case at dt 0.5
    cam = _camera(rng, 0, 48, 36)
    cases.append(Case("rgba16f u8", u8_standin(O, rng, (36, 44, 28)), cam, 48, 36, 0.5, random_table(rng, 256), (0.0, 1.0),
                      _light(O, rng, "headlight", cam), half=True))
    cases.append(Case("rgba16f f16", f16_edges(O, rng, (30, 26, 35)), cam, 48, 36, 0.5, random_table(rng, 17), (-0.5, 1.5), None, half=True))
    # colours at +-VK_TF_MAX_COLOUR, lit with every coefficient at 16 and the sharpest highlight
    cam = _camera(rng, 0, 40, 40)
    cases.append(Case("colours at the bound, lit at the bounds", u8_blobs(O, rng, (31, 42, 23)), cam, 40, 40, 0.5, big_table(rng, 256), (0.0, 1.0),
                      dict(direction=(0.3, -1.0, 0.2), ambient=16.0, diffuse=16.0, specular=16.0, shininess=1024.0)))
    cases.append(Case("colours at the bound, f16", f16_edges(O, rng, (27, 19, 33)), cam, 40, 40, 1.0, big_table(rng, 17), (-0.5, 1.5),
                      dict(direction="headlight", ambient=0.0, diffuse=16.0, specular=16.0, shininess=1.0)))
    return tuple(cases)


N_CASES = N_RANDOM + len(FIXED_DIMS) + 9


def cases(O):
    """The case list (deterministic: built once from SEED).  O: the oracle module (tests' `O` fixture)."""
    out = _cases(O)
    assert len(out) == N_CASES, len(out)
    return out
