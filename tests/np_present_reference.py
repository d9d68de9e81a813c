"""The present pass as it is specified (include/vokselis_hip.h: vk_present; DESIGN.md, "What the present pass computes"), in float64, and
the one comparison rule the present tests use.  Written from that text, not from the kernel or the C oracle.

Specification.  For pixel (x, y) of a w x h window over a bw x bh backbuffer, per channel:
- sample position and weights are an f32 chain and part of the specification: uv = (x + 0.5) / w, u = fma(uv, bw, -0.5), i = floor(u),
  f = u - i (kept below 1), taps i and i + 1 clamped to [0, bw - 1]; the same in y;
- both weights exactly 0: the value is texel (ix, iy) alone.  Otherwise a = t00 + fx (t10 - t00), b = t01 + fx (t11 - t01),
  v = a + fy (b - a) with IEEE semantics for the non-finite (NaN taps, inf - inf and 0 * inf make NaN);
- colour: s(A(v)), A(v) = clamp(v (2.51 v + 0.03) / (v (2.43 v + 0.59) + 0.14), 0, 1) extended by its limit (huge values and +-inf -> 1),
  s(c) = 12.92 c up to 0.0031308 and 1.055 c^0.41666 - 0.055 above; alpha: v itself; NaN -> 0 in every channel;
- q = 255 clamp(., 0, 1); the byte is floor(q + 0.5).  Bgra8 is Rgba8 with bytes 0 and 2 exchanged.
`present_q` returns q; `present_q32` evaluates the kernel's own f32 operation sequence in numpy (to measure how far f32 arithmetic may
stray from q: present_cases.DELTA); `judge` is the comparison rule."""
from __future__ import annotations

import numpy as np

f32, f64 = np.float32, np.float64
FRACT_MAX = f32(np.nextafter(f32(1.0), f32(0.0)))


def taps(n_out: int, n_in: int):
    """(i0, i1, f): the two clamped texel indices and the f32 weight of the second, for each of n_out samples along an axis of n_in texels."""
    x = np.arange(n_out, dtype=f32)
    uv = (x + f32(0.5)) / f32(n_out)                                   # one rounded add (exact below 2^23), one rounded division
    u = (uv.astype(f64) * f64(n_in) - 0.5).astype(f32)                 # fma: the product and the sum are exact in binary64, one rounding
    fl = np.floor(u)
    fr = np.minimum(u - fl, FRACT_MAX)                                 # u - floor(u) rounds to 1 for tiny negative u: fract stays below 1
    i = fl.astype(np.int64)
    return np.clip(i, 0, n_in - 1), np.clip(i + 1, 0, n_in - 1), fr


def sample(bb: np.ndarray, w: int, h: int) -> np.ndarray:
    """The blended value per output pixel and channel, float64 [h, w, 4], from the texels' exact values and the f32 weights."""
    with np.errstate(invalid="ignore"):  # (signalling NaN patterns are data here)
        t = np.asarray(bb).astype(f64)
    bh, bw = t.shape[:2]
    x0, x1, fx = taps(w, bw)
    y0, y1, fy = taps(h, bh)
    fx64, fy64 = fx.astype(f64)[None, :, None], fy.astype(f64)[:, None, None]
    t00, t10 = t[y0][:, x0], t[y0][:, x1]
    t01, t11 = t[y1][:, x0], t[y1][:, x1]
    with np.errstate(invalid="ignore", over="ignore"):
        a = t00 + fx64 * (t10 - t00)
        b = t01 + fx64 * (t11 - t01)
        v = a + fy64 * (b - a)
    centre = (fy == 0)[:, None, None] & (fx == 0)[None, :, None]
    return np.where(centre, t00, v)


def zero_weight_mask(w: int, h: int, bw: int, bh: int) -> np.ndarray:
    """[h, w] bool: samples whose two weights are both exactly 0."""
    return (taps(h, bh)[2] == 0)[:, None] & (taps(w, bw)[2] == 0)[None, :]


def aces(v):
    """ACESFilm on the extended reals, clamped to [0, 1]; NaN stays NaN.  Beyond |v| = 1e6 the ratio is written in 1 / v, which is the same
    function and reaches its limit 2.51 / 2.43 at +-inf."""
    v = np.asarray(v, f64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        big = np.abs(v) > 1e6
        vs = np.where(big, 1.0, v)
        r = np.where(big, 1.0 / np.where(big, v, 1.0), 0.0)
        small = vs * (2.51 * vs + 0.03) / (vs * (2.43 * vs + 0.59) + 0.14)
        large = (2.51 + 0.03 * r) / (2.43 + 0.59 * r + 0.14 * r * r)
        out = np.clip(np.where(big, large, small), 0.0, 1.0)
    return np.where(np.isnan(v), np.nan, out)


def srgb(c):
    c = np.asarray(c, f64)
    with np.errstate(invalid="ignore"):
        return np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 0.0031308), 0.41666) - 0.055)


def tone_q(v, alpha: bool = False):
    """q of a sampled value: the exact pre-rounding byte value."""
    v = np.asarray(v, f64)
    c = v if alpha else srgb(aces(v))
    with np.errstate(invalid="ignore"):
        c = np.clip(c, 0.0, 1.0)
    return 255.0 * np.where(np.isnan(c), 0.0, c)


def present_q(bb: np.ndarray, w: int, h: int) -> np.ndarray:
    """float64 [h, w, 4]: q for every output byte of presenting backbuffer bb ([bh, bw, 4], f16 or f32) to a w x h window."""
    v = sample(bb, w, h)
    q = np.empty_like(v)
    q[..., :3] = tone_q(v[..., :3])
    q[..., 3] = tone_q(v[..., 3], alpha=True)
    return q


# ---- the kernel's f32 operation sequence, in numpy float32 (for measuring DELTA; never a reference) -----------------------------------------

def _fma32(a, b, c):
    """fma(a, b, c) on f32 arrays: the product is exact in binary64, the sum rounds to binary64 and then to f32 (a double rounding that differs
    from the fused result in about one case in 2^29: immaterial for a worst-case measurement)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def present_q32(bb: np.ndarray, w: int, h: int) -> np.ndarray:
    """The f32 sequence of present_kernel / present_pack up to the rounding: three fma blends, ACESFilm term by term, exp2(log2(c) * 0.41666f),
    the clamp, * 255 + 0.5 -- minus that 0.5, as float64.  Where this strays from q, f32 arithmetic alone explains a wrong byte."""
    with np.errstate(invalid="ignore"):
        t = np.asarray(bb).astype(f32)
    bh, bw = t.shape[:2]
    x0, x1, fx = taps(w, bw)
    y0, y1, fy = taps(h, bh)
    fxb, fyb = np.broadcast_to(fx[None, :, None], (h, w, 4)), np.broadcast_to(fy[:, None, None], (h, w, 4))
    t00, t10 = t[y0][:, x0], t[y0][:, x1]
    t01, t11 = t[y1][:, x0], t[y1][:, x1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = _fma32(fxb, t10 - t00, t00)
        b = _fma32(fxb, t11 - t01, t01)
        v = np.where((fxb == 0) & (fyb == 0), t00, _fma32(fyb, b - a, a))
        x = v[..., :3]
        num = x * (f32(2.51) * x + f32(0.03))
        den = x * (f32(2.43) * x + f32(0.59)) + f32(0.14)
        c = np.where(np.abs(x) >= f32(1024.0), f32(1.0), num / den)
        c = np.where(np.isnan(c), f32(0.0), np.clip(c, f32(0.0), f32(1.0)))      # fmaxf(NaN, 0) = 0
        over = f32(1.055) * np.exp2(np.log2(c) * f32(0.41666)) - f32(0.055)
        s = np.where(c - f32(0.0031308) > 0, over, f32(12.92) * c)
        al = v[..., 3:]
        al = np.where(np.isnan(al), f32(0.0), al)
        z = np.clip(np.concatenate([s, al], axis=2), f32(0.0), f32(1.0)) * f32(255.0) + f32(0.5)
    return z.astype(f64) - 0.5


# ---- the comparison rule ------------------------------------------------------------------------------------------------------------------

def undecided(q, delta: float) -> np.ndarray:
    """Bytes whose q + 0.5 lies within delta of an integer: f32 arithmetic may land on either side."""
    z = np.asarray(q, f64) + 0.5
    return np.abs(z - np.round(z)) <= delta


def judge(got, q, delta: float):
    """(wrong, undecided): bool arrays.  A byte must equal floor(q + 0.5); where q + 0.5 lies within delta of an integer, the byte on either
    side of it is accepted.  Nothing else is: no "within one step"."""
    got = np.asarray(got).astype(np.int64)
    z = np.asarray(q, f64) + 0.5
    und = undecided(q, delta)
    lo, hi = np.floor(z - delta), np.floor(z + delta)
    ok = np.where(und, (got == np.clip(lo, 0, 255)) | (got == np.clip(hi, 0, 255)), got == np.floor(z))
    return ~ok, und


def bgra_of(rgba8: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(rgba8[..., [2, 1, 0, 3]])
