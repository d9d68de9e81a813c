"""The numpy reference of vk_volume_filter, on its own: whole-array np.float32 operations.  The three axis passes
gather their taps with clamped index arrays; the product of the first tap is an np.float32 multiply; the one fused operation
fmaf(w, t, acc) is formed as in tests/np_hist_reference.py -- the product is exact in float64, the sum is rounded to odd in float64 and then
once to f32, which equals the single rounding of the exact value because float64 carries more than two bits beyond f32 -- here with an
array as the addend, and with the non-finite cases (f16 volumes) left to float64's own arithmetic, whose infinities and NaNs arise exactly
where f32's do.  The store rule: np.rint of the clamped value for the integer formats, astype(np.float16) with NaN canonicalised for f16.
The median: np.partition over the 27 edge-padded shifts, on totalOrder keys for f16."""
import numpy as np

TOP = {"u8": 255.0, "u16": 65535.0}
DTYPE = {"u8": np.uint8, "u16": np.uint16, "f16": np.float16}
MAX_RADIUS, TAPS = 6, 13


def fmaf(w, t, c):
    """fmaf(w, t, c): w an np.float32 scalar, t and c np.float32 arrays."""
    a, b, c64 = np.asarray(t, np.float64), float(np.float32(w)), np.asarray(c, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                   # exact: 24 + 24 bits
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)           # TwoSum: p + c = s + err exactly
        fin = np.isfinite(s) & np.isfinite(p) & np.isfinite(c64)
        bits = s.view(np.int64)
        nudge = fin & (err != 0.0) & ((bits & 1) == 0)  # round to odd: an inexact sum takes the odd neighbour
        s = np.where(nudge, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def gaussian(sigma, radius):
    """vk_filter_gaussian's formula: exp in float64, the sum in the order of k, one rounding to f32."""
    g = [float(np.exp(-((k - radius) ** 2) / (2.0 * float(sigma) * float(sigma)))) for k in range(2 * radius + 1)]
    total = 0.0
    for v in g:
        total += v
    return np.array([v / total for v in g], np.float64).astype(np.float32)


def key16(bits):
    b = np.asarray(bits, np.uint16)
    return (b ^ np.where(b & np.uint16(0x8000), np.uint16(0xFFFF), np.uint16(0x8000))).astype(np.uint16)


def unkey16(key):
    k = np.asarray(key, np.uint16)
    return (k ^ np.where(k & np.uint16(0x8000), np.uint16(0x8000), np.uint16(0xFFFF))).astype(np.uint16)


def canonical(vol):
    """An f16 volume with every NaN as 0x7E00 (other kinds: unchanged)."""
    if vol.dtype != np.float16:
        return vol
    out = vol.copy()
    out.view(np.uint16)[np.isnan(vol)] = 0x7E00
    return out


def store(v, kind):
    """The store rule on an np.float32 array."""
    if kind == "f16":
        with np.errstate(over="ignore", invalid="ignore"):
            return canonical(v.astype(np.float16))
    return np.rint(np.minimum(np.maximum(v, np.float32(0.0)), np.float32(TOP[kind]))).astype(DTYPE[kind])


def convolve_f32(vol, radii, weights):
    """The unrounded f32 result of the three passes.  vol [nz, ny, nx]; radii (rx, ry, rz); weights [3][>= 2 r + 1]."""
    a = np.ascontiguousarray(vol).astype(np.float32)
    for axis, np_axis in ((0, 2), (1, 1), (2, 0)):
        r = int(radii[axis])
        if r == 0:
            continue
        w = np.asarray(weights[axis], np.float32)
        n = a.shape[np_axis]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = w[0] * np.take(a, np.clip(np.arange(n) - r, 0, n - 1), axis=np_axis)
        assert acc.dtype == np.float32
        for k in range(1, 2 * r + 1):
            acc = fmaf(w[k], np.take(a, np.clip(np.arange(n) - r + k, 0, n - 1), axis=np_axis), acc)
        a = acc
    return a


def convolve(vol, kind, radii, weights):
    return store(convolve_f32(vol, radii, weights), kind)


def median3(vol, kind):
    v = np.ascontiguousarray(vol)
    keys = key16(v.view(np.uint16)) if kind == "f16" else v
    nz, ny, nx = keys.shape
    p = np.pad(keys, 1, mode="edge")
    stack = np.stack([p[dz:dz + nz, dy:dy + ny, dx:dx + nx] for dz in range(3) for dy in range(3) for dx in range(3)])
    m = np.partition(stack, 13, axis=0)[13]
    return unkey16(m).view(np.float16) if kind == "f16" else m.astype(DTYPE[kind])


def neighbourhood(vol):
    """The 27 edge-clamped neighbours of every voxel, [27, nz, ny, nx]."""
    nz, ny, nx = vol.shape
    p = np.pad(vol, 1, mode="edge")
    return np.stack([p[dz:dz + nz, dy:dy + ny, dx:dx + nx] for dz in range(3) for dy in range(3) for dx in range(3)])


def apply(vol, kind, op, radii, weights):
    return median3(vol, kind) if op == "median3" else convolve(vol, kind, radii, weights)


def convolve_f64(vol, radii, weights):
    """The same three passes in float64 with the f32 weights: the yardstick of the 1 LSB property."""
    a = np.ascontiguousarray(vol).astype(np.float64)
    for axis, np_axis in ((0, 2), (1, 1), (2, 0)):
        r = int(radii[axis])
        if r == 0:
            continue
        w = np.asarray(weights[axis], np.float32).astype(np.float64)
        n = a.shape[np_axis]
        acc = np.zeros_like(a)
        for k in range(2 * r + 1):
            acc = acc + w[k] * np.take(a, np.clip(np.arange(n) - r + k, 0, n - 1), axis=np_axis)
        a = acc
    return a
