"""The rule of vk_volume_resample on whole arrays, written from the comment in include/vokselis_hip.h alone: np.float32 arithmetic, fmaf
spelled out through float64 (the product of two f32 is exact there; the sum is rounded to odd, so the second rounding to f32 is the
fused one), and beside it the float64 "definition" that rounds nowhere.  Arrays are [nz, ny, nx]; boxes (x0, y0, z0, x1, y1, z1)."""
import numpy as np

f32, f64 = np.float32, np.float64
DTYPE = {"u8": np.uint8, "u16": np.uint16, "f16": np.float16}
SCALE = {"u8": 255.0, "u16": 65535.0, "f16": 1.0}
MAX_RATIO = 16


def fmaf(x, y, z):
    """fmaf(x, y, z) over np.float32 arrays (broadcast)."""
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, c = np.asarray(x, f64), np.asarray(y, f64), np.asarray(z, f64)  # (a signalling NaN is quieted)
        p = a * b                                  # exact: 24 + 24 bits
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)             # TwoSum: p + c = s + err exactly
        fin = np.isfinite(s) & np.isfinite(p) & np.isfinite(c)
        bits = np.ascontiguousarray(s).view(np.int64)
        nudge = fin & (err != 0.0) & ((bits & 1) == 0)  # round to odd: an inexact sum takes the odd neighbour
        s = np.where(nudge, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(f32)


def crop(vol, box):
    x0, y0, z0, x1, y1, z1 = box
    return np.ascontiguousarray(vol[z0:z1, y0:y1, x0:x1])


def texels(sub):
    with np.errstate(invalid="ignore"):
        return sub.astype(f32)


def nearest_index(nb, n):
    j = np.arange(n, dtype=np.int64)
    return ((2 * j + 1) * nb) // (2 * n)


def linear_taps(nb, n):
    """(c(i), c(i + 1), f as float64 before its rounding to f32)."""
    j = np.arange(n, dtype=np.int64)
    num, den = (2 * j + 1) * nb - n, 2 * n
    i = num // den                                   # floor
    r = num - i * den
    return np.clip(i, 0, nb - 1), np.clip(i + 1, 0, nb - 1), r / f64(den)


def area_taps(nb, n):
    """(first, count, overlaps [n, max count] as int64, 0 beyond a voxel's count)."""
    j = np.arange(n, dtype=np.int64)
    first, last = (j * nb) // n, ((j + 1) * nb - 1) // n
    count = last - first + 1
    o = np.zeros((n, int(count.max())), np.int64)
    for c in range(o.shape[1]):
        k = first + c
        o[:, c] = np.where(c < count, np.minimum((j + 1) * nb, (k + 1) * n) - np.maximum(j * nb, k * n), 0)
    return first, count, o


def _lerp32(a, b, f):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(f == 0, a, fmaf(f, (b - a).astype(f32), a))


def _axis_shape(v, axis):
    s = [1, 1, 1]
    s[axis] = len(v)
    return np.asarray(v).reshape(s)


def _linear(t, nbs, ns, exact):
    for axis, nb, n in ((2, nbs[0], ns[0]), (1, nbs[1], ns[1]), (0, nbs[2], ns[2])):  # x, then y, then z
        i0, i1, f = linear_taps(nb, n)
        a, b = np.take(t, i0, axis), np.take(t, i1, axis)
        if exact:
            fa = _axis_shape(f, axis)
            with np.errstate(invalid="ignore", over="ignore"):
                t = np.where(fa == 0, a, a + fa * (b - a))
        else:
            t = _lerp32(a, b, _axis_shape(f.astype(f32), axis))
    return t


def _area(t, nbs, ns, exact):
    for axis, nb, n in ((2, nbs[0], ns[0]), (1, nbs[1], ns[1]), (0, nbs[2], ns[2])):
        first, count, o = area_taps(nb, n)
        w = o / f64(nb)
        if not exact:
            w = w.astype(f32)
        acc = None
        for c in range(o.shape[1]):
            live = _axis_shape(c < count, axis)
            tap = np.take(t, np.minimum(first + c, nb - 1), axis)
            wc = _axis_shape(w[:, c], axis)
            with np.errstate(invalid="ignore", over="ignore"):
                if c == 0:
                    acc = wc * tap if exact else (wc * tap).astype(f32)
                else:
                    acc = np.where(live, acc + wc * tap if exact else fmaf(wc, tap, acc), acc)
        t = acc
    return t


def value_map(kind_in, kind_out, window, exact=False):
    lo, hi = (0.0, 1.0) if window is None else (float(f32(window[0])), float(f32(window[1])))
    a, b = SCALE[kind_out] / ((hi - lo) * SCALE[kind_in]), -lo * SCALE[kind_out] / (hi - lo)
    with np.errstate(over="ignore"):
        return (a, b) if exact else (f32(a), f32(b))


def store(v, kind):
    """The store rule: f32 values into the stored type."""
    v = np.asarray(v, f32)
    if kind == "f16":
        with np.errstate(over="ignore", invalid="ignore"):
            h = v.astype(np.float16).view(np.uint16)  # round to nearest even, subnormals kept, overflow to infinity
        return np.where(np.isnan(v), np.uint16(0x7e00), h).astype(np.uint16).view(np.float16)
    top = f32(SCALE[kind])
    with np.errstate(invalid="ignore"):
        q = np.rint(np.fmin(np.fmax(v, f32(0)), top))     # ties to even
    return np.where(np.isnan(v), f32(0), q).astype(DTYPE[kind])


def refused(nbs, ns, mode):
    return mode == "area" and any(nb > MAX_RATIO * n for nb, n in zip(nbs, ns))


def resample(vol, kind, box, mode, dims, out_kind, window):
    """The library's output [nz, ny, nx] in the output's dtype."""
    sub = crop(vol, box)
    nbs = (sub.shape[2], sub.shape[1], sub.shape[0])
    assert min(nbs) > 0 and not refused(nbs, dims, mode)
    mapped = out_kind != kind or window is not None
    if mode == "nearest":
        ix, iy, iz = (nearest_index(nb, n) for nb, n in zip(nbs, dims))
        got = sub[np.ix_(iz, iy, ix)]
        if not mapped:
            return np.ascontiguousarray(got)
        v = texels(got)
    elif mode == "linear":
        v = _linear(texels(sub), nbs, dims, False)
    else:
        v = _area(texels(sub), nbs, dims, False)
    if mapped:
        a, b = value_map(kind, out_kind, window)
        v = fmaf(a, v, b)
    return np.ascontiguousarray(store(v, out_kind))


def definition(vol, kind, box, mode, dims, out_kind, window):
    """The value before the store in float64, nothing rounded to f32: what the rule approximates."""
    sub = crop(vol, box)
    nbs = (sub.shape[2], sub.shape[1], sub.shape[0])
    t = sub.astype(f64)
    if mode == "nearest":
        ix, iy, iz = (nearest_index(nb, n) for nb, n in zip(nbs, dims))
        v = t[np.ix_(iz, iy, ix)]
    elif mode == "linear":
        v = _linear(t, nbs, dims, True)
    else:
        v = _area(t, nbs, dims, True)
    if out_kind != kind or window is not None:
        a, b = value_map(kind, out_kind, window, True)
        with np.errstate(invalid="ignore", over="ignore"):
            v = a * v + b
    return v
