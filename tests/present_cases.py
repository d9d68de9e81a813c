"""The seeded fuzz cases of the present pass, shared by tests/test_present_fuzz_cpu.py (the C oracle's vo_present against the float64
reference of tests/np_present_reference.py) and tests/test_present_fuzz_gpu.py (vk_present, the fused epilogue and vk_capture_frame against
the same reference), so that both walk the same list.

A case is a backbuffer (its size, its format -- f16 or f32 -- and its content, as an array of that format) and a window size.  Sizes: equal;
non-integer up- and down-scales of each axis alone and of both; a 1 x 1 backbuffer under a larger window and a larger backbuffer under a
1 x 1 window; widths 63 / 64 / 65 (64 pixels x 4 B is capture_frame's row-pitch boundary); odd sizes; the largest windows vk_present accepts,
32768 x 1 and 1 x 32768.  Content: every f16 bit pattern once in each channel (in pattern order and shuffled); f32 edge values (+-0,
subnormals, the sRGB knee, both sides of each of the 255 rounding boundaries of colour and of alpha, 1, 65504, 1e10, the f32 neighbours of
the two points where ACESFilm's quadratics overflow, 1e30, +-inf, NaN patterns, negatives down to -1e30); log-uniform HDR noise over
1e-6 .. 1e5 with isolated inf / NaN texels and alpha other than 1.

Finite magnitudes stay <= 1e30, so no difference of two taps overflows in f32.  In every case that resamples (window != backbuffer) the
finite texels of a channel have one sign: the blend is then a convex combination.  Values of both signs side by side appear only in
equal-size cases, whose weights are 0, ~1e-7 or ~1 - 1e-7.

One more constraint, found while measuring DELTA (`tame`).  The pass blends as a + f (b - a), three fma.  b - a rounds to half an ulp of the
larger tap, so when f is close to 1 and |a| >> |b| the result, ~b + (1 - f) a, carries an absolute error of ~6e-8 |a|: a relative error of
~6e-8 / (1 - f), anything up to 50 % where f32 rounding puts a sample one ulp short of the next texel's centre (f = 1 - 6e-8, which happens in
equal-size presents of sizes that are not powers of two: the sample 38620 -> 0.0107 at f = 0.99999994 is 0.0130 exactly and 0.0146 in f32).
That is the arithmetic the pass is specified with (it is the form a GPU sampler's lerp has too), not a fault to chase, and no tolerance
expresses it; so wherever a sample has 1 - f < 1/16 along an axis, the texel that carries the vanishing weight is redrawn within a factor
two of its neighbour's magnitude (its sign and every non-finite texel kept).  The blend's relative error is then ~1e-6 at most, the size of
the tone map's own f32 error, and DELTA measures both.

DELTA, the half-width of the comparison rule's undecided band (np_present_reference.judge), is four times MEASURED_MAX, the largest
|q32 - q| over the finite q of this whole list, q32 being the kernel's f32 operation sequence evaluated in numpy float32
(np_present_reference.present_q32); the factor covers the 1-ulp v_exp_f32 / v_log_f32 against libm.  test_present_fuzz_cpu.py measures it
again and holds it to the figure written here."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import np_present_reference as R

SEED = 20261016
# Measured over this list (test_present_fuzz_cpu.py::test_delta_is_four_times_the_measured_f32_error prints it): see the note beside DELTA in
# DESIGN.md.  8.27e-5 measured, rounded up.
MEASURED_MAX = 8.5e-5
DELTA = 4.0 * MEASURED_MAX
F32_NAN_BITS = (0x7FC00000, 0x7F800001, 0xFFC00000, 0xFF800001, 0x7FFFFFFF)
ALPHAS = (1.0, 0.0, 0.5, 2.0, -1.0, np.nan)
# alpha 0.5 is q = 127.5 exactly, an undecided byte by construction (either neighbour is accepted): it is kept rare
ALPHA_HALF_SHARE = 0.004


@dataclass
class Case:
    name: str
    bb: np.ndarray             # [bh, bw, 4] float16 or float32: the backbuffer's content
    w: int
    h: int
    tags: tuple = field(default_factory=tuple)

    @property
    def half(self):
        return self.bb.dtype == np.float16

    @property
    def bw(self):
        return self.bb.shape[1]

    @property
    def bh(self):
        return self.bb.shape[0]

    @property
    def resamples(self):
        return (self.w, self.h) != (self.bw, self.bh)

    def __repr__(self):
        return f"Case({self.name}: {self.bw}x{self.bh} {'rgba16f' if self.half else 'rgba32f'} -> {self.w}x{self.h})"


# ---- edge values ----

def _bisect(fn, target, lo, hi):
    """x in [lo, hi] with fn(x) = target, fn non-decreasing (float64 bisection to the last bit)."""
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if fn(mid) < target:
            lo = mid
        else:
            hi = mid
    return lo, hi


def _colour_q(x):
    return float(R.tone_q(np.float64(x)))


def _f32_at_most(fn, x, bound):
    """The largest f32 <= x with fn(f32) <= bound."""
    v = np.float32(x)
    while fn(float(v)) > bound:
        v = np.nextafter(v, np.float32(-np.inf))
    return v


def _f32_at_least(fn, x, bound):
    v = np.float32(x)
    while fn(float(v)) < bound:
        v = np.nextafter(v, np.float32(np.inf))
    return v


@functools.lru_cache(maxsize=None)
def boundary_values():
    """(colour, alpha): f32 values on both sides of each of the 255 rounding boundaries q = k + 0.5, each the f32 nearest to its boundary
    among those at least 2 DELTA away from it (by the float64 reference), so that none of them is undecided."""
    colour, alpha = [], []
    for k in range(255):
        t = k + 0.5
        lo, hi = _bisect(_colour_q, t, 0.0, 8.0)
        colour.append(_f32_at_most(_colour_q, lo, t - 2.0 * DELTA))
        colour.append(_f32_at_least(_colour_q, hi, t + 2.0 * DELTA))
        qa = lambda a: 255.0 * a
        alpha.append(_f32_at_most(qa, t / 255.0, t - 2.0 * DELTA))
        alpha.append(_f32_at_least(qa, t / 255.0, t + 2.0 * DELTA))
    return np.array(colour, np.float32), np.array(alpha, np.float32)


def overflow_points():
    """The smallest f32 x at which ACESFilm's numerator x (2.51 x + 0.03), and its denominator, is inf in f32 arithmetic: between the two the
    quotient is inf / finite (white); from the second on it was inf / inf = NaN (black) before the curve was extended by its limit."""
    out = []
    with np.errstate(over="ignore"):
        for k in (np.float32(2.51), np.float32(2.43)):
            lo, hi = np.float32(1e18), np.float32(1e20)
            while np.nextafter(lo, hi) < hi:
                mid = np.float32(0.5 * (np.float64(lo) + np.float64(hi)))
                if np.isinf(mid * (k * mid)):
                    hi = mid
                else:
                    lo = mid
            out.append(hi)
    return tuple(out)


def _neighbours(x, n=2):
    x = np.float32(x)
    out, up, dn = [x], x, x
    for _ in range(n):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        out += [up, dn]
    return out


@functools.lru_cache(maxsize=None)
def edge_values():
    """(non-negative finite, negative finite, non-finite) f32 edge values, NaNs as their bit patterns."""
    lo, hi = _bisect(lambda x: float(R.aces(np.float64(x))), 0.0031308, 0.0, 1.0)  # the input whose tone-mapped value is the sRGB knee
    n_over, d_over = overflow_points()
    pos = [0.0, 1e-45, 1e-40, 1.17549435e-38, 1e-6, 1.0, 7.0, 7.3, 8.0, 1023.0, 1024.0, 1025.0, 65504.0, 65520.0, 1e10, 1e18, 1e30]
    pos += _neighbours(lo, 3) + _neighbours(n_over) + _neighbours(d_over)
    neg = [-0.0, -1e-45, -1e-40, -1e-3, -0.03 / 2.51, -0.1, -0.2429, -0.25, -1.0, -1023.0, -1024.0, -65504.0, -1e10, -1e30]
    neg += [-v for v in _neighbours(n_over)] + [-v for v in _neighbours(d_over)]
    nonfinite = np.concatenate([np.array([np.inf, -np.inf], np.float32), np.array(F32_NAN_BITS, np.uint32).view(np.float32)])
    return np.array(pos, np.float32), np.array(neg, np.float32), nonfinite


# ---- content ----

def _alpha(rng, pool, shape):
    """Alpha drawn evenly from the pool, but +-0.5 with probability ALPHA_HALF_SHARE (at least one texel, where there are four or more)."""
    pool = np.array(pool, np.float32)
    half = np.abs(pool) == 0.5
    rest, halves = pool[~half], pool[half]
    al = rest[rng.integers(0, len(rest), shape)]
    if len(halves):
        m = rng.random(shape) < ALPHA_HALF_SHARE
        if al.size >= 4:
            m.flat[int(rng.integers(0, al.size))] = True
        al[m] = halves[rng.integers(0, len(halves), int(m.sum()))]
    return al


def _fill(rng, bw, bh, pool, channel_alpha=None):
    """[bh, bw, 4] f32 drawn from `pool` per colour channel (every value of the pool at least once where there is room, dealt at a different
    offset per channel), alpha from channel_alpha."""
    n = bw * bh
    bb = np.empty((bh, bw, 4), np.float32)
    for c in range(3):
        idx = np.concatenate([rng.permutation(len(pool)), rng.integers(0, len(pool), max(0, n - len(pool)))])[:n]
        bb[..., c] = pool[rng.permutation(idx)].reshape(bh, bw)
    bb[..., 3] = _alpha(rng, ALPHAS if channel_alpha is None else channel_alpha, (bh, bw))
    return bb


def hdr_noise(rng, bw, bh, signs=(1, 1, 1), alpha=None, half=False):
    """Log-uniform noise over 1e-6 .. 1e5 times the channel's sign, ~3 % isolated non-finite texels per channel, alpha from `alpha`."""
    bb = np.empty((bh, bw, 4), np.float32)
    for c in range(3):
        bb[..., c] = signs[c] * 10.0 ** rng.uniform(-6.0, 5.0, (bh, bw))
    bb[..., 3] = _alpha(rng, ALPHAS if alpha is None else alpha, (bh, bw))
    nonfinite = edge_values()[2]
    for c in range(3):
        m = rng.random((bh, bw)) < 0.03
        bb[..., c][m] = nonfinite[rng.integers(0, len(nonfinite), int(m.sum()))]
    if bw * bh >= 4:  # at least one +inf, -inf and NaN texel, wherever the draw fell
        where = rng.choice(bw * bh, 3, replace=False)
        for j, v in enumerate(nonfinite[:3]):
            bb[..., j].flat[where[j]] = v
    with np.errstate(over="ignore", invalid="ignore"):  # beyond 65504 a half is +inf, as on an rgba16f surface
        return bb.astype(np.float16) if half else bb


def f16_patterns(rng, shuffled):
    """256 x 256 rgba16f: every f16 bit pattern once in each channel.  In pattern order the channels are offset against each other (a
    swapped channel shows); shuffled, each channel has its own permutation, so that non-finite texels have finite neighbours."""
    p = np.arange(65536, dtype=np.uint32)
    if shuffled:
        chans = [rng.permutation(p) for _ in range(4)]
    else:
        chans = [p, 65535 - p, (p + 0x4000) & 0xFFFF, (p + 0x8000) & 0xFFFF]
    return np.stack([c.astype(np.uint16).reshape(256, 256) for c in chans], axis=2).view(np.float16)


def tame(rng, bb, w, h, t=1.0 / 16.0):
    """bb with the texels that carry a vanishing weight (1 - f < t for some sample of a w x h window, along either axis) redrawn within a factor
    two of the magnitude of the texel that carries the rest: see the module's text.  Signs and non-finite texels stay."""
    with np.errstate(invalid="ignore"):
        out = np.array(bb, np.float32)
    bh, bw = out.shape[:2]
    for axis, (n_out, n_in) in ((1, (w, bw)), (0, (h, bh))):
        i0, i1, f = R.taps(n_out, n_in)
        flagged = np.unique(i0[(f > 1.0 - t) & (i1 == i0 + 1)])
        for i in flagged[::-1]:  # from the far end: the neighbour is final before it is used
            a, b = (out[:, i], out[:, i + 1]) if axis == 1 else (out[i], out[i + 1])
            ok = np.isfinite(a) & np.isfinite(b)
            with np.errstate(invalid="ignore"):
                new = np.copysign(np.abs(b) * rng.uniform(0.5, 2.0, a.shape).astype(np.float32), a)
                a[ok] = np.clip(new, np.float32(-1e30), np.float32(1e30))[ok]
    if bb.dtype == np.float16:  # the texels left alone convert back to their own bits
        with np.errstate(over="ignore", invalid="ignore"):
            return np.where(out == bb.astype(np.float32), bb, out.astype(np.float16))
    return out


# ---- the list ----

EQUAL = ((63, 5), (64, 4), (65, 3), (17, 31), (1, 1), (2, 1), (1, 2))
RESAMPLE = (
    # (backbuffer, window, tag)
    ((40, 30), (57, 30), "x up"), ((40, 30), (40, 43), "y up"), ((40, 30), (27, 30), "x down"), ((40, 30), (40, 19), "y down"),
    ((37, 23), (101, 77), "both up"), ((96, 96), (95, 33), "both down"), ((33, 47), (66, 94), "x2"), ((64, 32), (32, 16), "half"),
    ((1, 1), (13, 7), "1x1 backbuffer"), ((9, 11), (1, 1), "1x1 window"), ((9, 11), (1, 8), "1xN window"),
    ((50, 7), (63, 5), "width 63"), ((50, 7), (64, 5), "width 64"), ((50, 7), (65, 5), "width 65"),
    ((7, 5), (32768, 1), "32768x1"), ((5, 7), (1, 32768), "1x32768"),
)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(SEED)
    pos, neg, nonfinite = edge_values()
    bcol, balpha = boundary_values()
    out = []
    # every f16 pattern, at its own size: every sample has zero weights (256 is a power of two), the rows before the +-inf rows included
    out.append(Case("f16 patterns in order", f16_patterns(rng, False), 256, 256, ("patterns",)))
    out.append(Case("f16 patterns shuffled", f16_patterns(rng, True), 256, 256, ("patterns",)))
    # both sides of every rounding boundary, colour and alpha: equal size (each value presented as itself) -- no undecided byte
    bb = np.empty((16, 32, 4), np.float32)  # 510 values and two repeats; powers of two: every sample has zero weights
    for c in range(3):
        bb[..., c] = np.roll(np.concatenate([bcol, bcol[:2]]), 37 * c).reshape(16, 32)
    bb[..., 3] = np.concatenate([balpha, balpha[:2]]).reshape(16, 32)
    out.append(Case("rounding boundaries", bb, 32, 16, ("boundaries",)))
    # all edge values of both signs and the non-finite side by side: equal sizes only
    everything = np.concatenate([pos, neg, nonfinite])
    for bw, bh in EQUAL + ((16, 16),):
        out.append(Case(f"edges {bw}x{bh}", tame(rng, _fill(rng, bw, bh, everything), bw, bh), bw, bh, ("edges",)))
        out.append(Case(f"noise {bw}x{bh} f16", tame(rng, hdr_noise(rng, bw, bh, signs=(1, -1, 1), half=True), bw, bh), bw, bh, ("noise",)))
    with np.errstate(invalid="ignore"):
        mixed = hdr_noise(rng, 16, 16) * np.where(rng.random((16, 16, 4)) < 0.5, -1, 1).astype(np.float32)
    out.append(Case("noise 16x16 f32, mixed signs", mixed, 16, 16, ("noise",)))
    with np.errstate(invalid="ignore"):
        mixed = hdr_noise(rng, 21, 13) * np.where(rng.random((13, 21, 4)) < 0.5, -1, 1).astype(np.float32)
    out.append(Case("noise 21x13 f32, mixed signs", tame(rng, mixed, 21, 13), 21, 13, ("noise",)))
    # resampling: one sign per channel among the finite texels
    pos_alpha, neg_alpha = np.array([1.0, 0.0, 0.5, 2.0, np.nan], np.float32), np.array([-1.0, -0.0, -0.5, -2.0, np.nan], np.float32)
    for j, ((bw, bh), (w, h), tag) in enumerate(RESAMPLE):
        signs = ((1, 1, 1), (1, -1, 1), (-1, -1, -1))[j % 3]
        alpha = neg_alpha if j % 4 == 3 else pos_alpha
        out.append(Case(f"noise {tag} f32", tame(rng, hdr_noise(rng, bw, bh, signs, alpha), w, h), w, h, ("noise", tag)))
        out.append(Case(f"noise {tag} f16", tame(rng, hdr_noise(rng, bw, bh, signs[::-1], alpha, half=True), w, h), w, h, ("noise", tag)))
        pool = np.concatenate([neg if j % 2 else pos, nonfinite])
        out.append(Case(f"edges {tag} f32", tame(rng, _fill(rng, bw, bh, pool, neg_alpha if j % 2 else pos_alpha), w, h), w, h, ("edges", tag)))
    return tuple(out)


N_CASES = 3 + 2 * (len(EQUAL) + 1) + 2 + 3 * len(RESAMPLE)


def one_sign(case) -> bool:
    """The finite texels of every channel have one sign (zeros of either sign count for both)."""
    with np.errstate(invalid="ignore"):
        v = case.bb.astype(np.float64)
    fin = np.isfinite(v)
    return all(not ((v[..., c][fin[..., c]] > 0).any() and (v[..., c][fin[..., c]] < 0).any()) for c in range(4))
