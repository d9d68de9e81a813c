"""An independent reference for first-hit isosurface rendering (vk_set_isosurface), written from DESIGN.md section 14 and
include/vokselis_hip.h, not from tests/iso_restatement.c: vectorised numpy.

Ray generation, intersect_box and the trilinear sample (f32, fma emulated) are oracle/np_restatement.py's.  What decides a ray's fate is
exact in f32: the hit test x >= iso_k per sample (a NaN sample is no hit), and the bisection -- m = a + 2^-i, q = fma(-m, s, p) per
component, the sample at q against iso_k.  What only moves colour is evaluated in float64 (tests/np_table_reference.py's gradient and
shade): the gradient of the interpolant at q = fma(-a, s, p) from its eight taps, its normalisation, |N.L|, the half vector, |N.H|^n,
and linear_to_srgb.

It also counts, per ray, the iterations whose cell is not empty under the isosurface's predicate, restated here: a cell is empty iff its
eight (clamped) taps are finite and its largest tap lies below iso_k."""
from __future__ import annotations

import numpy as np

from oracle import np_restatement as R

from np_table_reference import FLT_MIN, _gradient, _shade, light_dir, srgb64

f32 = np.float32


def iso_k(iso, r8):
    with np.errstate(over="ignore"):  # (a finite iso may overflow to +-inf on R8)
        return f32(iso) * f32(255.0) if r8 else f32(iso)


def cells_empty(taps, k):
    """The isosurface's predicate over arrays of eight taps (f32, on the kernel's scale)."""
    t = np.stack([np.asarray(v, np.float32) for v in taps])
    finite = np.isfinite(t).all(axis=0)
    M = np.max(np.where(np.isfinite(t), t, f32(0.0)), axis=0)
    return finite & (M < k)


def _back(m, s, p):
    return R.fma((-m).astype(np.float32), s, p)


def render(camera_blob: bytes, vol: np.ndarray, W: int, H: int, *, iso, colour=(1.0, 1.0, 1.0), refine=4, dt=1.0, light=None, tile=None):
    """Returns (rgb float64 [H, W, 3], steps u32 [H, W], nonempty u32 [H, W]: the iterations whose cell is not empty, hit bool [H, W],
    a f32 [H, W]: the refined distance back); pixels outside the tile, and rays that miss the box, are 0 with 0 steps."""
    with np.errstate(invalid="ignore", over="ignore"):
        return _render(camera_blob, vol, W, H, iso, colour, refine, dt, light, tile)


def _render(camera_blob, vol, W, H, iso, colour, refine, dt, light, tile):
    vol = np.ascontiguousarray(vol)
    r8 = vol.dtype == np.uint8
    nz, ny, nx = vol.shape
    rgb_out = np.zeros((H, W, 3), np.float64)
    steps_out = np.zeros((H, W), np.uint32)
    live_out = np.zeros((H, W), np.uint32)
    hit_out = np.zeros((H, W), bool)
    a_out = np.zeros((H, W), np.float32)
    ray = R.naive_rays(camera_blob, (nx, ny, nz), W, H, dt, tile)
    if ray is None:
        return rgb_out, steps_out, live_out, hit_out, a_out
    xs, ys, d, box, t0, t1, dtv, p, st = (ray[k] for k in ("xs", "ys", "d", "hit", "t0", "t1", "dt", "p", "st"))
    k = iso_k(iso, r8)
    nr = box.size
    t = t0.copy()
    nst = np.zeros(nr, np.uint32)
    live = np.zeros(nr, np.uint32)
    hit = np.zeros(nr, bool)
    active = box & (t < t1)
    while active.any():
        idx = np.nonzero(active)[0]
        x, _, taps, _ = R.sample_trilinear(vol, [p[c][idx] for c in range(3)], raw=True, taps=True)
        nst[idx] += 1
        live[idx] += (~cells_empty(taps, k)).astype(np.uint32)
        h = x >= k
        hit[idx[h]] = True
        cont = idx[~h]  # a hit leaves p where the hit sample was taken
        for c in range(3):
            p[c][cont] = (p[c][cont] + st[c][cont]).astype(np.float32)
        t[cont] = (t[cont] + dtv[cont]).astype(np.float32)
        active[idx[h]] = False
        active[cont] = t[cont] < t1[cont]
    # the bisection, on the rays that hit after their first iteration
    a = np.zeros(nr, np.float32)
    ref = np.nonzero(hit & (nst >= 2))[0]
    for i in range(1, int(refine) + 1):
        if ref.size == 0:
            break
        m = (a[ref] + f32(2.0 ** -i)).astype(np.float32)
        q = [_back(m, st[c][ref], p[c][ref]) for c in range(3)]
        x = R.sample_trilinear(vol, q, raw=True, taps=True)[0]
        a[ref] = np.where(x >= k, m, a[ref])
    # the shade at q = fma(-a, s, p), once per ray that hit
    hi = np.nonzero(hit)[0]
    rgb = [np.full(hi.size, float(f32(c))) for c in colour]
    if light is not None and hi.size:
        q = [_back(a[hi], st[c][hi], p[c][hi]) for c in range(3)]
        _, _, taps, fr = R.sample_trilinear(vol, q, raw=True, taps=True)
        g = _gradient(taps, fr, (nx, ny, nz))
        V = [-np.asarray(c, np.float64)[hi] for c in d]
        if isinstance(light["direction"], str):
            Ld = V
        else:
            l3 = light_dir(light["direction"])
            Ld = [np.full(hi.size, l3[c]) for c in range(3)]
        hv = [Ld[c] + V[c] for c in range(3)]
        hq = hv[0] * hv[0] + hv[1] * hv[1] + hv[2] * hv[2]
        ok = hq >= FLT_MIN
        hs = 1.0 / np.sqrt(np.where(ok, hq, 1.0))
        Hd = [np.where(ok, hv[c] * hs, V[c]) for c in range(3)]
        rgb = _shade(rgb, g, Ld, Hd, light)
    out = np.zeros((3, nr), np.float64)
    out[:, hi] = srgb64(np.stack(rgb))
    rgb_out[np.ix_(ys, xs)] = out.T.reshape(ys.size, xs.size, 3)
    steps_out[np.ix_(ys, xs)] = nst.reshape(ys.size, xs.size)
    live_out[np.ix_(ys, xs)] = live.reshape(ys.size, xs.size)
    hit_out[np.ix_(ys, xs)] = hit.reshape(ys.size, xs.size)
    a_out[np.ix_(ys, xs)] = a.reshape(ys.size, xs.size)
    return rgb_out, steps_out, live_out, hit_out, a_out
