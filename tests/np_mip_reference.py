"""An independent reference for the maximum-intensity projection (vk_set_projection(VK_PROJ_MAX)), written from DESIGN.md section 12 and
include/vokselis_hip.h, not from tests/mip_restatement.c: vectorised numpy.

Ray generation, intersect_box and the trilinear sample (f32, fma emulated) are oracle/np_restatement.py's.  The running maximum is exact:
u = min(max(fma(x, k1, k2), 0), n - 1) per sample in f32 (a NaN sample gives 0), U the largest of them -- a maximum rounds nothing.  The
ray ends after the iteration in which U reaches n - 1.  The lookup (i = min(floor(U), n - 2), the lerp of T[i] and T[i + 1]) and
linear_to_srgb are evaluated in float64.

It also counts, per ray, the iterations whose cell is not empty under the projection's predicate, restated here: a cell is empty iff its
eight (clamped) taps are finite and its largest tap M has min(max(fma(M, k1, k2), 0), n - 1) == 0."""
from __future__ import annotations

import numpy as np

from oracle import np_restatement as R

from np_table_reference import srgb64, tf_constants

f32 = np.float32
GREY_RAMP = np.array([[0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]], np.float32)


def tf_u(x, k1, k2, umax):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.fmin(np.fmax(R.fma(x, k1, k2), f32(0.0)), umax)  # fmax drops a NaN


def cells_empty(taps, k1, k2, umax):
    """The MAX predicate over arrays of eight taps (f32, on the kernel's scale)."""
    t = np.stack([np.asarray(v, np.float32) for v in taps])
    finite = np.isfinite(t).all(axis=0)
    with np.errstate(invalid="ignore"):
        M = np.where(finite, np.max(np.where(np.isfinite(t), t, f32(0.0)), axis=0), f32(0.0))
    return finite & (tf_u(M, k1, k2, umax) == 0)


def render(camera_blob: bytes, vol: np.ndarray, W: int, H: int, *, table=None, domain=(0.0, 1.0), dt=1.0, tile=None):
    """Returns (rgb float64 [H, W, 3], steps u32 [H, W], nonempty u32 [H, W]: the iterations whose cell is not empty); pixels outside
    the tile are 0 with 0 steps, rays that miss the box are 0 with 0 steps."""
    with np.errstate(invalid="ignore", over="ignore"):
        return _render(camera_blob, vol, W, H, table, domain, dt, tile)


def _render(camera_blob, vol, W, H, table, domain, dt, tile):
    vol = np.ascontiguousarray(vol)
    r8 = vol.dtype == np.uint8
    nz, ny, nx = vol.shape
    rgb_out = np.zeros((H, W, 3), np.float64)
    steps_out = np.zeros((H, W), np.uint32)
    live_out = np.zeros((H, W), np.uint32)
    ray = R.naive_rays(camera_blob, (nx, ny, nz), W, H, dt, tile)
    if ray is None:
        return rgb_out, steps_out, live_out
    xs, ys, hit, t0, t1, dtv, p, st = (ray[k] for k in ("xs", "ys", "hit", "t0", "t1", "dt", "p", "st"))
    if table is None:
        table, domain = GREY_RAMP, (0.0, 1.0)
    T64 = np.ascontiguousarray(table, np.float32).astype(np.float64)
    n = T64.shape[0]
    k1, k2 = tf_constants(n, domain[0], domain[1], r8)
    umax = f32(n - 1)
    nr = hit.size
    U = np.zeros(nr, np.float32)
    t = t0.copy()
    nst = np.zeros(nr, np.uint32)
    live = np.zeros(nr, np.uint32)
    active = hit & (t < t1)
    while active.any():
        idx = np.nonzero(active)[0]
        x, _, taps, _ = R.sample_trilinear(vol, [p[k][idx] for k in range(3)], raw=True, taps=True)
        nst[idx] += 1
        live[idx] += (~cells_empty(taps, k1, k2, umax)).astype(np.uint32)
        U[idx] = np.maximum(U[idx], tf_u(x, k1, k2, umax))
        done = U[idx] >= umax
        cont = idx[~done]
        for k in range(3):
            p[k][cont] = (p[k][cont] + st[k][cont]).astype(np.float32)
        t[cont] = (t[cont] + dtv[cont]).astype(np.float32)
        active[idx[done]] = False
        active[cont] = t[cont] < t1[cont]
    U64 = U.astype(np.float64)
    i = np.minimum(np.floor(U64).astype(np.int64), n - 2)
    f = U64 - i
    c = np.stack([T64[i, k] + f * (T64[i + 1, k] - T64[i, k]) for k in range(3)])
    out = np.where(hit[None, :], srgb64(c), 0.0)
    rgb_out[np.ix_(ys, xs)] = out.T.reshape(ys.size, xs.size, 3)
    steps_out[np.ix_(ys, xs)] = nst.reshape(ys.size, xs.size)
    live_out[np.ix_(ys, xs)] = live.reshape(ys.size, xs.size)
    return rgb_out, steps_out, live_out
