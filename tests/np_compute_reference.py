"""A second, independent reference for the compute twin (VK_MODE_COMPUTE_NEAREST: raycast_compute.wgsl's render / get_col2): vectorised
numpy, written from the shader text and DESIGN.md section 4.3, not from the C oracle.

The ray set-up is oracle/np_restatement.py's compute_rays.  What decides the step counts stays in f32 as the shader has it: t and its
additions t = t + dt, the sample position p = eye + t * dir and its voxel (truncation of (p + 1) * dims / 2), the opacity
smoothstep(0, 0.7, a^3) with the specified a * a * a and reciprocal form, w = (1 - A) * opacity, A += w and the early-out A >= 0.95.
Everything that only moves colour is float64: the shade max(0, dot((0, -1, 0), n)), the directional light max(dot(n, l1), 0) *
smoothstep(0.3, 1.5, dot(p, l2)), mix(shade, bl * (0, 0, 0.6), 0.2), col = rgb + 3 * (1, 0.1, 0.13) * dl * ss, and the compositing
C += w * col * shade + clear.rgb * clear.a * (1 - opacity).  Every term the text writes is evaluated, so NaN appears where the text's
arithmetic gives one: 0 * inf inside a dot product, an infinite colour or shade times a zero weight.  max / min drop a NaN operand (fmax /
fmin), as the design specifies.  Out-of-range loads read zeros."""
from __future__ import annotations

import numpy as np

from oracle import np_restatement as R

f32 = np.float32
CLEAR = (0.023, 0.02, 0.02, 0.0)


def opacity(a):
    """smoothstep(0, 0.7, a * a * a) in f32: s = (x - 0) * (1 / 0.7), clamped with fmin / fmax (a NaN gives 0), then s * s * (3 - 2 s) with
    the last factor one fma."""
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((a * a).astype(np.float32) * a).astype(np.float32)
    s = ((x - f32(0.0)) * (f32(1.0) / (f32(0.7) - f32(0.0)))).astype(np.float32)
    s = np.fmin(np.fmax(s, f32(0.0)), f32(1.0))
    return ((s * s).astype(np.float32) * R.fma(f32(-2.0), s, f32(3.0))).astype(np.float32)


def _smoothstep64(e0, e1, x):
    s = np.fmin(np.fmax((x - e0) / (e1 - e0), 0.0), 1.0)
    return s * s * (3.0 - 2.0 * s)


def _unit64(v):
    v = np.array(v, np.float64)
    return v / np.sqrt((v * v).sum())


L1 = _unit64((-2.0, -2.0, -1.0))
L2 = _unit64((1.0, 1.0, -1.0))


def render(camera_blob: bytes, den: np.ndarray, nrm: np.ndarray, W: int, H: int, *, dt=1.0, tile=None):
    """get_col2 over `tile` (default: the full frame; any origin).  den, nrm: f16 [nz, ny, nx, 4].  Returns (rgb float64 [H, W, 3],
    steps u32 [H, W]); pixels outside the tile are 0 with 0 steps, rays that miss the box the clear colour with 0 steps."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):  # (non-finite data propagates as the text says)
        return _render(camera_blob, den, nrm, W, H, dt, tile)


def _render(camera_blob, den, nrm, W, H, dt_scale, tile):
    nz, ny, nx = den.shape[:3]
    rgb_out = np.zeros((H, W, 3), np.float64)
    steps_out = np.zeros((H, W), np.uint32)
    ray = R.compute_rays(camera_blob, (nx, ny, nz), W, H, dt_scale, tile)
    if ray is None:
        return rgb_out, steps_out
    xs, ys, eye, d, hit, t0, t1, dt, hb = (ray[k] for k in ("xs", "ys", "eye", "d", "hit", "t0", "t1", "dt", "hb"))
    den64 = den.astype(np.float64)
    nrm64 = nrm.astype(np.float64)
    den32 = den.astype(np.float32)
    nr = hit.size
    C = np.tile(np.array(CLEAR[:3], np.float64)[:, None], (1, nr))
    A = np.full(nr, f32(0.1), np.float32)
    t = t0.copy()
    nst = np.zeros(nr, np.uint32)
    active = hit & (t < t1)
    while active.any():
        idx = np.nonzero(active)[0]
        tt = t[idx]
        p = [(eye[k][idx] + (tt * d[k][idx]).astype(np.float32)).astype(np.float32) for k in range(3)]
        v = [np.trunc(((p[k] + f32(1.0)).astype(np.float32) * hb[k]).astype(np.float32)) for k in range(3)]
        v = [np.nan_to_num(c, nan=0.0, posinf=1 << 30, neginf=-(1 << 30)).astype(np.int64) for c in v]
        inb = (v[0] >= 0) & (v[1] >= 0) & (v[2] >= 0) & (v[0] < nx) & (v[1] < ny) & (v[2] < nz)
        jx, jy, jz = (np.clip(v[k], 0, n - 1) for k, n in enumerate((nx, ny, nz)))
        a32 = np.where(inb, den32[jz, jy, jx, 3], f32(0.0)).astype(np.float32)
        rgb = np.where(inb[:, None], den64[jz, jy, jx, :3], 0.0)
        n = np.where(inb[:, None], nrm64[jz, jy, jx, :3], 0.0)
        nst[idx] += 1
        va = opacity(a32)
        w = ((f32(1.0) - A[idx]) * va).astype(np.float32)
        # colour, float64: every term of the text
        sh = np.fmax(0.0, (0.0 * n[:, 0] + -1.0 * n[:, 1]) + 0.0 * n[:, 2])
        dl = np.fmax((n[:, 0] * L1[0] + n[:, 1] * L1[1]) + n[:, 2] * L1[2], 0.0)
        p64 = [c.astype(np.float64) for c in p]
        ss = _smoothstep64(0.3, 1.5, (p64[0] * L2[0] + p64[1] * L2[1]) + p64[2] * L2[2])
        bl = 0.9 * np.fmin(np.fmax(0.5 - 0.5 * n[:, 1], 0.0), 1.0)
        w64, va64 = w.astype(np.float64), va.astype(np.float64)
        for k, (lc, blc) in enumerate(zip((1.0, 0.1, 0.13), (0.0, 0.0, 0.6))):
            col = rgb[:, k] + 3.0 * lc * dl * ss
            shade = sh * (1.0 - 0.2) + (bl * blc) * 0.2
            C[k, idx] = (C[k, idx] + w64 * col * shade) + CLEAR[k] * CLEAR[3] * (1.0 - va64)
        A[idx] = (A[idx] + (w * (f32(1.0) - f32(CLEAR[3]))).astype(np.float32)).astype(np.float32)
        done = A[idx] >= f32(0.95)
        cont = idx[~done]
        t[cont] = (t[cont] + dt[cont]).astype(np.float32)
        active[idx[done]] = False
        active[cont] = t[cont] < t1[cont]
    out = np.where(hit[None, :], C, np.array(CLEAR[:3], np.float64)[:, None])
    rgb_out[np.ix_(ys, xs)] = out.T.reshape(ys.size, xs.size, 3)
    steps_out[np.ix_(ys, xs)] = nst.reshape(ys.size, xs.size)
    return rgb_out, steps_out
