"""The numpy reference of vk_volume_histogram, on its own: the constants from the request in float64 rounded once to
f32, the texels of the box as np.float32, the classification with np.float32 comparisons, the one fused operation fmaf(t, k1, k2) as a
correctly rounded f32 (the product is exact in float64; the sum is rounded to odd in float64 and then once to f32, which equals the single
rounding of the exact value because float64 carries more than two bits beyond f32), min and max in the order of the ordered integer key
(-0 below +0), and the sums EXACTLY, as fractions (every finite texel of the three formats is an integer multiple of 2^-24), against which
the f64 sums of the restatement and of the kernels are held."""
from fractions import Fraction

import numpy as np

SCALE = {"u8": 255.0, "u16": 65535.0, "f16": 1.0}


def constants(kind, lo, hi, bins):
    """lo_k, hi_k, k1, k2 as np.float32 (vk_hist.hpp: hist_validate)."""
    lo, hi, S = float(np.float32(lo)), float(np.float32(hi)), SCALE[kind]
    span = hi - lo
    return np.float32(lo * S), np.float32(hi * S), np.float32(bins / (span * S)), np.float32(-lo * bins / span)


def fmaf(t, k1, k2):
    """fmaf over an array of finite np.float32 t with finite scalars k1, k2."""
    a, b, c = np.asarray(t, np.float64), float(k1), float(k2)
    p = a * b                                 # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)           # TwoSum: p + c = s + err exactly
    bits = s.view(np.int64)
    nudge = (err != 0.0) & ((bits & 1) == 0)  # round to odd: an inexact sum takes the odd neighbour
    s = np.where(nudge, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def key(t):
    """The order-preserving u32 key of f32 values."""
    b = np.asarray(t, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def texels(vol, box=None):
    """The box's texels as a flat np.float32 array in x-fastest order.  vol: [nz, ny, nx] of uint8 / uint16 / float16."""
    nz, ny, nx = vol.shape
    (x0, y0, z0), (x1, y1, z1) = ((0, 0, 0), (nx, ny, nz)) if box is None else box
    return np.ascontiguousarray(vol[z0:z1, y0:y1, x0:x1]).astype(np.float32).ravel()


def histogram(vol, kind, bins, domain, box=None):
    """dict(counts u64 [bins], n_voxels, n_nan, n_below, n_above, n_finite, min f32, max f32, sum, sum_sq, abs_sum (exact Fractions))."""
    lo_k, hi_k, k1, k2 = constants(kind, domain[0], domain[1], bins)
    t = texels(vol, box)
    nan = np.isnan(t)
    with np.errstate(invalid="ignore"):
        below = ~nan & (t < lo_k)
        above = ~nan & (t > hi_k)
    inr = ~(nan | below | above)
    u = np.floor(fmaf(t[inr], k1, k2))
    b = np.clip(u, 0, bins - 1).astype(np.int64)
    counts = np.bincount(b, minlength=bins).astype(np.uint64)
    real = t[~nan]
    if real.size:
        k = key(real)
        mn, mx = real[int(np.argmin(k))], real[int(np.argmax(k))]
    else:
        mn, mx = np.float32(np.inf), np.float32(-np.inf)
    fin = t[np.isfinite(t)].astype(np.float64)
    units = [int(v) for v in fin * 2.0 ** 24]  # exact: a half's smallest subnormal is 2^-24
    assert all(float(v) == w for v, w in zip(units[:64], (fin * 2.0 ** 24)[:64]))
    return dict(counts=counts, n_voxels=int(t.size), n_nan=int(nan.sum()), n_below=int(below.sum()), n_above=int(above.sum()), n_finite=int(fin.size),
                min=np.float32(mn), max=np.float32(mx), sum=Fraction(sum(units), 2 ** 24), sum_sq=Fraction(sum(v * v for v in units), 2 ** 48),
                abs_sum=Fraction(sum(abs(v) for v in units), 2 ** 24))


def sum_bound(n, abs_sum):
    """The standard bound of an f64 sum of n terms, in any order, against the exact sum: (n - 1) * 2^-53 * sum(|x|), as a Fraction."""
    return Fraction(max(n - 1, 0), 2 ** 53) * abs_sum


def sum_error(got, exact):
    """|got - exact| of an f64 against a Fraction, exactly."""
    return abs(Fraction(float(got)) - exact)
