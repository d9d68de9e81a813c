"""A second, independent reference for the table march (vk_set_transfer_function) and the lit table march
(vk_set_lighting, section 10): vectorised numpy, written from the design and include/vokselis_hip.h, not from the C restatements
(tests/tf_restatement.c, tests/lit_restatement.c).

Ray generation, intersect_box and the trilinear sample are oracle/np_restatement.py's, which is itself independent of the C oracle.
What decides the step counts stays in f32, fma emulated as np_restatement.fma does: the sample, the table coordinate
u = min(max(fma(x, k1, k2), 0), n - 1), i = min(floor(u), n - 2), f = u - i, the alpha lerp, w = (1 - A) a and A += w, and the early-out
A >= 0.95.  Everything that only moves colour is evaluated in float64: the colour lerp, the gradient (the analytic derivative of the
trilinear interpolant, from the taps), its normalisation, |N.L|, the half vector, |N.H|^n, the compositing of G and linear_to_srgb.
The restatements round each of those operations to f32 in the kernels' order; this one does not share that order, so the two agree
within a tolerance, with step counts equal."""
from __future__ import annotations

import math

import numpy as np

from oracle import np_restatement as R

f32 = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def tf_constants(n, lo, hi, r8):
    """k1 = (n-1) / ((hi-lo) S), k2 = -lo (n-1) / (hi-lo) with lo, hi as f32, computed in double and rounded once (S = 255 for u8)."""
    lo, hi = float(f32(lo)), float(f32(hi))
    span, nm1 = hi - lo, float(n) - 1.0
    return f32(nm1 / (span * (255.0 if r8 else 1.0))), f32(-lo * nm1 / span)


def light_dir(direction):
    """The world light as the host stores it: the f32 direction normalised in double, each component rounded once to f32."""
    x, y, z = (float(f32(v)) for v in direction)
    n = math.sqrt(x * x + y * y + z * z)
    return np.array([float(f32(x / n)), float(f32(y / n)), float(f32(z / n))])


def srgb64(x):
    """linear_to_srgb in float64: 12.92 x up to 0.0031308, 1.055 x^(1/2.4) - 0.055 above."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        hi = 1.055 * np.power(np.maximum(x, 1e-30), 1.0 / 2.4) - 0.055
    return np.where(x <= 0.0031308, 12.92 * x, hi)


def _gradient(t, fr, dims):
    """World gradient (float64) of the trilinear interpolant at weights fr = (fx, fy, fz), from the eight taps t."""
    T = [np.asarray(v, np.float64) for v in t]
    fx, fy, fz = (np.asarray(v, np.float64) for v in fr)
    with np.errstate(invalid="ignore", over="ignore"):
        # d/dx: the y-z bilinear blend of the four x-differences
        dx = [T[1] - T[0], T[3] - T[2], T[5] - T[4], T[7] - T[6]]
        e0, e1 = dx[0] + fy * (dx[1] - dx[0]), dx[2] + fy * (dx[3] - dx[2])
        gx = e0 + fz * (e1 - e0)
        # d/dy: the z blend of the y-differences of the x-lerps
        c00, c10, c01, c11 = T[0] + fx * dx[0], T[2] + fx * dx[1], T[4] + fx * dx[2], T[6] + fx * dx[3]
        gy = (c10 - c00) + fz * ((c11 - c01) - (c10 - c00))
        # d/dz: the difference of the two y-lerps
        gz = (c01 + fy * (c11 - c01)) - (c00 + fy * (c10 - c00))
    return gx * dims[0], gy * dims[1], gz * dims[2]


def _shade(rgb, g, Ld, Hd, light):
    """rgb' = c.rgb (ka + kd diff) + ks spec; diff = |N.L|, spec = |N.H|^n with a gradient (q finite and >= FLT_MIN), 1 and 0 without."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
        has = (q >= FLT_MIN) & (q <= FLT_MAX)
        s = 1.0 / np.sqrt(np.where(has, q, 1.0))
        N = [gi * s for gi in g]
        nl = np.abs(N[0] * Ld[0] + N[1] * Ld[1] + N[2] * Ld[2])
        nh = np.abs(N[0] * Hd[0] + N[1] * Hd[1] + N[2] * Hd[2])
        diff = np.where(has, nl, 1.0)
        spec = np.where(has, np.power(np.where(has, nh, 0.0), float(f32(light["shininess"]))), 0.0)
    ka, kd, ks = (float(f32(light[k])) for k in ("ambient", "diffuse", "specular"))
    f = ka + kd * diff
    return [c * f + ks * spec for c in rgb]


def render(camera_blob: bytes, vol: np.ndarray, W: int, H: int, *, table, domain=(0.0, 1.0), dt=1.0, light=None, tile=None):
    """The table march (light: the keyword arguments of Context.set_lighting, or None) over `tile` (default: the full frame; any origin).
    Returns (rgb float64 [H, W, 3], steps u32 [H, W]); pixels outside the tile, and rays that miss the box, are 0 with 0 steps."""
    with np.errstate(invalid="ignore", over="ignore"):  # (non-finite taps are data here: they propagate as the design says)
        return _render(camera_blob, vol, W, H, table, domain, dt, light, tile)


def _render(camera_blob, vol, W, H, table, domain, dt, light, tile):
    vol = np.ascontiguousarray(vol)
    r8 = vol.dtype == np.uint8
    nz, ny, nx = vol.shape
    rgb_out = np.zeros((H, W, 3), np.float64)
    steps_out = np.zeros((H, W), np.uint32)
    ray = R.naive_rays(camera_blob, (nx, ny, nz), W, H, dt, tile)
    if ray is None:
        return rgb_out, steps_out
    xs, ys, d, hit, t0, t1, dtv, p, st = (ray[k] for k in ("xs", "ys", "d", "hit", "t0", "t1", "dt", "p", "st"))
    T32 = np.ascontiguousarray(table, np.float32)
    T64 = T32.astype(np.float64)
    n = T32.shape[0]
    k1, k2 = tf_constants(n, domain[0], domain[1], r8)
    umax, imax = f32(n - 1), n - 2
    nr = hit.size
    # per ray: the light and the half vector (float64, from the f32 direction)
    if light is not None:
        V = [-np.asarray(c, np.float64) for c in d]
        if isinstance(light["direction"], str):
            Ld = V
        else:
            l3 = light_dir(light["direction"])
            Ld = [np.full(nr, l3[k]) for k in range(3)]
        h = [Ld[k] + V[k] for k in range(3)]
        hq = h[0] * h[0] + h[1] * h[1] + h[2] * h[2]
        ok = hq >= FLT_MIN
        hs = 1.0 / np.sqrt(np.where(ok, hq, 1.0))
        Hd = [np.where(ok, h[k] * hs, V[k]) for k in range(3)]
    G = np.zeros((3, nr), np.float64)
    A = np.zeros(nr, np.float32)
    t = t0.copy()
    nst = np.zeros(nr, np.uint32)
    with np.errstate(invalid="ignore"):
        active = hit & (t < t1)
    while active.any():
        idx = np.nonzero(active)[0]
        pa = [p[k][idx] for k in range(3)]
        x, _, taps, fr = R.sample_trilinear(vol, pa, raw=True, taps=True)
        nst[idx] += 1
        with np.errstate(invalid="ignore", over="ignore"):
            u = np.fmin(np.fmax(R.fma(x, k1, k2), f32(0.0)), umax)  # fmax drops a NaN: a NaN sample reads entry 0
        i = np.minimum(np.floor(u).astype(np.int64), imax)
        f = (u - i.astype(np.float32)).astype(np.float32)
        a = R.fma(f, (T32[i + 1, 3] - T32[i, 3]).astype(np.float32), T32[i, 3])
        f64 = f.astype(np.float64)
        rgb = [T64[i, k] + f64 * (T64[i + 1, k] - T64[i, k]) for k in range(3)]
        if light is not None:
            g = _gradient(taps, fr, (nx, ny, nz))
            rgb = _shade(rgb, g, [c[idx] for c in Ld], [c[idx] for c in Hd], light)
        w = ((f32(1.0) - A[idx]) * a).astype(np.float32)
        w64 = w.astype(np.float64)
        for k in range(3):
            G[k, idx] += w64 * rgb[k]
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
    return rgb_out, steps_out
