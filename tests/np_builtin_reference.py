"""A second, independent reference for the built-in transfer function of VK_MODE_NAIVE_TRILINEAR (no table): vectorised numpy, written
from the design (raycast_naive.wgsl's transfer and palette as SURVEY Appendix A specifies them), not from the C
oracle.

Ray generation is oracle/np_restatement.py's naive_rays, the taps and weights its sample_trilinear's.  What decides the step counts stays
in f32, fma emulated as np_restatement.fma does: the filter (x, then y, then z, each lerp one fma), transfer_alpha with fmin semantics
(min(NaN, c) = c), w = (1 - A) a, A += w and the early-out A >= 0.95.  Everything that only moves colour is evaluated in float64: the
palette vertigo(alpha), the compositing and linear_to_srgb.  The count of sampled steps uses this module's own restatement of the
skip maps' predicate (cell_empty), which tests/builtin_fuzz.cpp ties to the library's vk_tf.hpp."""
from __future__ import annotations

import numpy as np

from np_table_reference import srgb64
from oracle import np_restatement as R

f32 = np.float32


def tap_empty(t, f16):
    """The built-in emptiness of a tap (f32 value on the kernel's scale: u8 0..255, f16 the value): u8 t <= 25; f16 finite and t <= 0.1."""
    t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore"):
        return (np.isfinite(t) & (t <= f32(0.1))) if f16 else (t <= f32(25.0))


def cell_empty(taps, f16):
    """A cell is empty when all eight of its taps are."""
    out = np.ones(np.shape(taps[0]), bool)
    for t in taps:
        out &= tap_empty(t, f16)
    return out


def lerp(a, b, f):
    return R.fma(f, (b - a).astype(np.float32), a)


def filter_taps(t, fr):
    """The trilinear filter in f32: x, then y, then z, each lerp fma(f, b - a, a)."""
    c00, c10, c01, c11 = lerp(t[0], t[1], fr[0]), lerp(t[2], t[3], fr[0]), lerp(t[4], t[5], fr[0]), lerp(t[6], t[7], fr[0])
    return lerp(lerp(c00, c10, fr[1]), lerp(c01, c11, fr[1]), fr[2])


def transfer_alpha(x, r8):
    """smoothstep(0.1, 1.2, min(v, 0.9)) in f32 with the affine map as one fma whose constants carry the scale of x (r8: filtered taps on
    0..255, c = 229.5, k1 = 1/(255 * 1.1); f16: the value, c = 0.9, k1 = 1/1.1); k2 = -0.1/1.1.  fmin drops a NaN: alpha(NaN) = alpha(c)."""
    c = f32(229.5) if r8 else f32(0.9)
    k1 = f32(1.0 / (255.0 * 1.1)) if r8 else f32(1.0 / 1.1)
    s = R.fma(np.fmin(np.asarray(x, np.float32), c), k1, f32(-0.1 / 1.1))
    s = np.fmin(np.fmax(s, f32(0.0)), f32(1.0))
    return ((s * s).astype(np.float32) * R.fma(f32(-2.0), s, f32(3.0))).astype(np.float32)


def vertigo64(a):
    """The palette 0.5 + 0.5 cos(6.28318 (c a + d)), c = (1, 1.7, 0.4), d = (0, 0.15, 0.2), in float64."""
    a = np.asarray(a, np.float64)
    return [0.5 + 0.5 * np.cos(6.28318 * (c * a + d)) for c, d in ((1.0, 0.0), (1.7, 0.15), (0.4, 0.2))]


def render(camera_blob: bytes, vol: np.ndarray, W: int, H: int, *, dt=1.0, tile=None, on_sample=None):
    """The built-in march over `tile` (default: the full frame; any origin).  Returns (rgb float64 [H, W, 3], steps u32 [H, W], sampled
    u32 [H, W]: the steps in a cell that cell_empty calls not empty); pixels outside the tile, and rays that miss the box, are 0 with 0
    steps.  on_sample(alpha f32, empty bool), if given, sees every sample's alpha with its cell's emptiness."""
    with np.errstate(invalid="ignore", over="ignore"):  # (non-finite taps are data here: they propagate as the design says)
        return _render(camera_blob, np.ascontiguousarray(vol), W, H, dt, tile, on_sample)


def _render(camera_blob, vol, W, H, dt, tile, on_sample):
    r8, f16 = vol.dtype == np.uint8, vol.dtype == np.float16
    nz, ny, nx = vol.shape
    rgb_out = np.zeros((H, W, 3), np.float64)
    steps_out = np.zeros((H, W), np.uint32)
    sampled_out = np.zeros((H, W), np.uint32)
    ray = R.naive_rays(camera_blob, (nx, ny, nz), W, H, dt, tile)
    if ray is None:
        return rgb_out, steps_out, sampled_out
    xs, ys, hit, t0, t1, dtv, p, st = (ray[k] for k in ("xs", "ys", "hit", "t0", "t1", "dt", "p", "st"))
    nr = hit.size
    G = np.zeros((3, nr), np.float64)
    A = np.zeros(nr, np.float32)
    t = t0.copy()
    nst = np.zeros(nr, np.uint32)
    nsm = np.zeros(nr, np.uint32)
    active = hit & (t < t1)
    while active.any():
        idx = np.nonzero(active)[0]
        _, _, taps, fr = R.sample_trilinear(vol, [p[k][idx] for k in range(3)], raw=True, taps=True)
        a = transfer_alpha(filter_taps(taps, fr), r8)
        empty = cell_empty(taps, f16)
        if on_sample is not None:
            on_sample(a, empty)
        nst[idx] += 1
        nsm[idx] += (~empty).astype(np.uint32)
        w = ((f32(1.0) - A[idx]) * a).astype(np.float32)
        w64 = w.astype(np.float64)
        for k, c in enumerate(vertigo64(a)):
            G[k, idx] += w64 * c
        A[idx] = (A[idx] + w).astype(np.float32)
        done = A[idx] >= f32(0.95)
        cont = idx[~done]
        for k in range(3):
            p[k][cont] = (p[k][cont] + st[k][cont]).astype(np.float32)
        t[cont] = (t[cont] + dtv[cont]).astype(np.float32)
        active[idx[done]] = False
        active[cont] = t[cont] < t1[cont]
    out = np.where(hit[None, :], srgb64(G), 0.0)
    rgb_out[np.ix_(ys, xs)] = out.T.reshape(ys.size, xs.size, 3)
    steps_out[np.ix_(ys, xs)] = nst.reshape(ys.size, xs.size)
    sampled_out[np.ix_(ys, xs)] = nsm.reshape(ys.size, xs.size)
    return rgb_out, steps_out, sampled_out
