"""The shared case list of the volume filter tests (vk_volume_filter): small volumes of the three formats and for each
a set of filters.  The CPU suite holds the C restatement to the numpy reference over it (tests/test_filter_fuzz_cpu.py), the GPU suite
every layout's kernels to the restatement (tests/test_filter_fuzz_gpu.py).  A volume is shared by its filters (`vol_id`): the GPU driver
uploads it once per layout.

The dimensions follow the kernels' tile shapes (vokselis_amd/csrc/vk_filter.hpp; TILES below, held to that file by the CPU suite): on
every axis a dimension of 1, one below the largest radius + 1, one equal to a tile edge, a tile edge + 1, one that spans two tiles and a
remainder, and odd ones (the clamped last cell of the PACKED layouts)."""
from collections import namedtuple

import numpy as np

import np_filter_reference as NF

Case = namedtuple("Case", "name vol_id kind vol op radii weights")

TILES = ((32, 8, 8, 2), (32, 8, 8, 4), (32, 4, 4, 6))  # tx, ty, tz, largest radius: the convolve classes
MEDIAN_TILE = (32, 8, 8, 1)
DIMS = ((1, 1, 1), (2, 1, 3), (5, 7, 3), (8, 8, 8), (33, 9, 10), (70, 19, 18), (16, 16, 16), (37, 5, 1), (32, 4, 4), (32, 9, 9), (9, 5, 5))  # nx, ny, nz
MAX_VOXELS = 25000
MAX_WEIGHT = 1024.0

DYADIC = np.array([0.25, 0.5, 0.25], np.float32)
DYADIC5 = np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)
SHARPEN = np.array([-1.0, 3.0, -1.0], np.float32)
EXTREME5 = np.array([MAX_WEIGHT, -MAX_WEIGHT, MAX_WEIGHT, -MAX_WEIGHT, MAX_WEIGHT], np.float32)
EXTREME3 = np.array([-MAX_WEIGHT, MAX_WEIGHT, MAX_WEIGHT], np.float32)


def _filters():
    """(name, op, radii, weights): weights [3] of arrays (None: radius 0)."""
    g = NF.gaussian
    out = [
        ("identity, all radii 0", "convolve", (None, None, None)),
        ("dyadic x", "convolve", (DYADIC, None, None)),
        ("dyadic y", "convolve", (None, DYADIC, None)),
        ("dyadic z", "convolve", (None, None, DYADIC)),
        ("dyadic x y", "convolve", (DYADIC, DYADIC, None)),
        ("dyadic y z, 5 taps", "convolve", (None, DYADIC5, DYADIC5)),
        ("dyadic x y z", "convolve", (DYADIC, DYADIC, DYADIC)),
        ("asymmetric radii (1, 0, 6)", "convolve", (DYADIC, None, g(2.0, 6))),
        ("asymmetric radii (5, 2, 0)", "convolve", (g(1.7, 5), g(0.8, 2), None)),
        ("asymmetric radii (0, 6, 0)", "convolve", (None, g(2.5, 6), None)),
        ("Gaussian sigma 0.8 radius 2", "convolve", (g(0.8, 2), g(0.8, 2), g(0.8, 2))),
        ("Gaussian radii (3, 4, 3)", "convolve", (g(1.0, 3), g(1.3, 4), g(1.0, 3))),
        ("Gaussian sigma 0.5 radius 6, the maximum radius on every axis", "convolve", (g(0.5, 6), g(0.5, 6), g(0.5, 6))),
        ("Gaussian sigma 2 radius 6, the maximum radius on every axis", "convolve", (g(2.0, 6), g(2.0, 6), g(2.0, 6))),
        ("sharpen, negative weights", "convolve", (SHARPEN, SHARPEN, SHARPEN)),
        ("weights at +-MAX_WEIGHT", "convolve", (EXTREME5, None, EXTREME3)),
        ("MEDIAN3", "median3", (None, None, None)),
    ]
    return [(n, op, tuple(0 if x is None else len(x) // 2 for x in w), w) for n, op, w in out]


FILTERS = _filters()
EVERY_DIMS = ("identity, all radii 0", "Gaussian sigma 2 radius 6, the maximum radius on every axis", "MEDIAN3")


def shape(d):
    return (d[2], d[1], d[0])


def _cast(x, kind, scale):
    """Values in [0, 1] onto the format's range."""
    if kind == "f16":
        return x.astype(np.float16)
    return np.rint(np.clip(x, 0.0, 1.0) * scale).astype(NF.DTYPE[kind])


def ball(d, kind):
    nz, ny, nx = shape(d)
    z, y, x = np.meshgrid((np.arange(nz) + 0.5) / nz, (np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    r = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    return _cast(np.clip(1.3 - 3.2 * r, 0.0, 1.0), kind, NF.TOP.get(kind, 1.0))


def f16_specials():
    return [np.float16(np.nan), np.float16(np.inf), np.float16(-np.inf), np.float16(-0.0), np.float16(0.0), np.float16(6e-8), np.float16(-6e-8), np.float16(3e-5),
            np.float16(65504.0), np.float16(-65504.0), np.float16(1.0), np.float16(-2.5)]


def volumes():
    """(vol_id, kind, vol [nz, ny, nx]): per format the data kinds of the issue, the dimensions in rotation."""
    rng = np.random.default_rng(22)
    out, k = [], 0

    def dims(n=2):
        nonlocal k
        picked = [DIMS[(k + 5 * j) % len(DIMS)] for j in range(n)]
        k += 1
        return picked

    for kind in ("u8", "u16", "f16"):
        top = NF.TOP.get(kind, 1.0)
        hi = 256 if kind == "u8" else 65536
        for d in dims():
            out.append((f"{kind} {d} constant", kind, _cast(np.full(shape(d), 77.0 / 255.0), kind, top)))
        for d in dims():
            out.append((f"{kind} {d} two-valued", kind, _cast(rng.choice(np.array([0.125, 0.875]), shape(d), p=(0.8, 0.2)), kind, top)))
        for d in dims(3):
            v = rng.uniform(-2.0, 2.0, shape(d)).astype(np.float16) if kind == "f16" else rng.integers(0, hi, shape(d)).astype(NF.DTYPE[kind])
            out.append((f"{kind} {d} uniform", kind, v))
        for d in dims():
            out.append((f"{kind} {d} ball", kind, ball(d, kind)))
        for d in dims():
            v = np.zeros(shape(d), NF.DTYPE[kind])
            flat = v.reshape(-1)
            flat[::29] = NF.DTYPE[kind](1.0 if kind == "f16" else hi - 56)  # lone speckles in zeros: at least 28 voxels apart along x
            out.append((f"{kind} {d} lone speckles in zeros", kind, v))
        for d in dims():
            sat = rng.choice(np.array([0.0, 1.0]), shape(d))
            out.append((f"{kind} {d} saturating, 0 and the top", kind, (sat * 65504.0).astype(np.float16) if kind == "f16" else _cast(sat, kind, top)))
    for d in ((70, 19, 18), (5, 7, 3), (33, 9, 10)):
        v = rng.normal(0.5, 0.4, shape(d)).astype(np.float16)
        flat = v.reshape(-1)
        sp = f16_specials()
        for rep in range(max(1, flat.size // 400)):
            for j, s in enumerate(sp):
                flat[(rep * 397 + j * 31 + 3) % flat.size] = s
        flat[-1] = np.float16(-0.0)  # the last voxel of an odd dimension
        out.append((f"f16 {d} normal with NaN, inf, -0, denormals", "f16", v))
    out.append(("f16 (9, 5, 5) denormals only", "f16", (rng.integers(-40, 41, shape((9, 5, 5))) * 2.0 ** -24).astype(np.float16)))
    out.append(("f16 (2, 1, 3) all NaN", "f16", np.full(shape((2, 1, 3)), np.nan, np.float16)))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        out, k = [], 0
        rest = [f for f in FILTERS if f[0] not in EVERY_DIMS]
        for vol_id, kind, vol in volumes():
            take = 4 if "uniform" in vol_id or "NaN" in vol_id else 3
            for j in range(take):
                name, op, radii, weights = rest[(k + j) % len(rest)]
                out.append(Case(f"{vol_id}, {name}", vol_id, kind, vol, op, radii, weights))
            k += take
            if "uniform" in vol_id or "speckles" in vol_id or "NaN" in vol_id or "denormals only" in vol_id:
                for name, op, radii, weights in FILTERS:
                    if name in EVERY_DIMS and not any(c.vol_id == vol_id and c.name.endswith(name) for c in out):
                        out.append(Case(f"{vol_id}, {name}", vol_id, kind, vol, op, radii, weights))
        # every dimension under the identity, the maximum radius and the median, on u8 data that saturates and ties
        rng = np.random.default_rng(23)
        for d in DIMS:
            vol = rng.integers(0, 256, shape(d)).astype(np.uint8)
            for name, op, radii, weights in FILTERS:
                if name in EVERY_DIMS or name == "sharpen, negative weights":
                    out.append(Case(f"u8 {d} uniform (every dimension), {name}", f"u8 {d} uniform (every dimension)", "u8", vol, op, radii, weights))
        _CASES = out
    return _CASES


def weights_array(c):
    """The [3][13] float32 array of a case's request (unused entries 0)."""
    w = np.zeros((3, NF.TAPS), np.float32)
    for a in range(3):
        if c.weights[a] is not None:
            w[a, :len(c.weights[a])] = c.weights[a]
    return w
