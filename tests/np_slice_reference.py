"""An independent reference for the slice pass (vk_render_slice), written from DESIGN.md section 19 and include/vokselis_hip.h, not from
tests/slice_restatement.c: vectorised numpy over the whole frame.

Positions, the inside test, the taps (from the dense array, clamp-to-edge), the filter and the three reductions are formed in f32 with
numpy operations (an fma is the f64 product and sum rounded once to f32: oracle/np_restatement.py's fma), in the specified order, so P,
inside and x are the specification's bits.  The lookup and linear_to_srgb are evaluated in float64."""
from __future__ import annotations

import numpy as np

from oracle.np_restatement import fma

from np_table_reference import srgb64

f32 = np.float32
SCALE = {np.dtype(np.uint8): 255.0, np.dtype(np.float16): 1.0, np.dtype(np.uint16): 65535.0}
GREY_RAMP = np.array([[0.0, 0.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0]], np.float32)


def trilinear(vol, p):
    """The filtered sample of a [nz, ny, nx] volume at positions p = (x, y, z) arrays: u = fma(q, n, -0.5), floor, fract, texel indices
    clamped to the edge, the x-lerps, then y, then z, each lerp fma(f, b - a, a)."""
    nz, ny, nx = vol.shape
    dims = (nx, ny, nz)
    fr, i0, i1 = [], [], []
    for a in range(3):
        u = fma(p[a], f32(dims[a]), f32(-0.5))
        fl = np.floor(u)
        f = (u - fl).astype(np.float32)
        f = np.where(f >= f32(1.0), np.nextafter(f32(1.0), f32(0.0)), f)  # the device's fract stays below 1
        ii = np.clip(fl.astype(np.float64), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)  # the saturating conversion
        fr.append(f)
        i0.append(np.clip(ii, 0, dims[a] - 1))
        i1.append(np.clip(np.minimum(ii + 1, 2 ** 31 - 1), 0, dims[a] - 1))

    def tap(ix, iy, iz):
        return vol[iz, iy, ix].astype(np.float32)

    def lerp(a, b, f):
        return fma(f, (b - a).astype(np.float32), a)

    t = [tap(i0[0], i0[1], i0[2]), tap(i1[0], i0[1], i0[2]), tap(i0[0], i1[1], i0[2]), tap(i1[0], i1[1], i0[2]),
         tap(i0[0], i0[1], i1[2]), tap(i1[0], i0[1], i1[2]), tap(i0[0], i1[1], i1[2]), tap(i1[0], i1[1], i1[2])]
    c00, c10, c01, c11 = lerp(t[0], t[1], fr[0]), lerp(t[2], t[3], fr[0]), lerp(t[4], t[5], fr[0]), lerp(t[6], t[7], fr[0])
    return lerp(lerp(c00, c10, fr[1]), lerp(c01, c11, fr[1]), fr[2])


def positions(plane, W, H):
    """P of every pixel: fma((float)py, dv.c, fma((float)px, du.c, origin.c)), three [H, W] f32 arrays."""
    plane = np.asarray(plane, np.float32)
    px, py = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return [fma(py, plane[2][c], fma(px, plane[1][c], plane[0][c])) for c in range(3)]


def value(vol, P, plane, samples, reduce):
    """x at positions P (arrays of one shape): the sample, or the slab's reduction in the order of k."""
    plane = np.asarray(plane, np.float32)
    if samples == 1:
        return trilinear(vol, P)
    M = np.full(P[0].shape, {"max": -np.inf, "min": np.inf, "mean": 0.0}[reduce], np.float32)
    half = f32(0.5) * f32(samples - 1)
    for k in range(samples):
        w = f32(f32(k) - half)
        xk = trilinear(vol, [fma(w, plane[3][c], P[c]) for c in range(3)])
        if reduce == "max":
            M = np.where(xk > M, xk, M)
        elif reduce == "min":
            M = np.where(xk < M, xk, M)
        else:
            M = (M + xk).astype(np.float32)
    if reduce == "mean":
        M = (M * f32(1.0 / float(samples))).astype(np.float32)
    return M


def render(vol, W, H, plane, *, samples=1, reduce="max", table=None, domain=(0.0, 1.0), box=None, tile=None):
    """Returns (rgb float64 [H, W, 3], val f32 [H, W, 2], pos f32 [H, W, 3], inside bool [H, W]).  Pixels outside the tile: colour 0, the
    zero record, position 0, not inside."""
    with np.errstate(invalid="ignore", over="ignore"):
        return _render(np.ascontiguousarray(vol), W, H, plane, samples, reduce, table, domain, box, tile)


def _render(vol, W, H, plane, samples, reduce, table, domain, box, tile):
    P = positions(plane, W, H)
    lo, hi = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)) if box is None else box
    inside = np.ones((H, W), bool)
    for c in range(3):
        inside &= (f32(lo[c]) <= P[c]) & (P[c] <= f32(hi[c]))
    if tile is not None:
        tx, ty, tw, th = tile
        m = np.zeros((H, W), bool)
        m[max(ty, 0):max(ty + th, 0), max(tx, 0):max(tx + tw, 0)] = True
        inside &= m
        P = [np.where(m, p, f32(0.0)) for p in P]
    rgb, val = np.zeros((H, W, 3), np.float64), np.zeros((H, W, 2), np.float32)
    pos = np.stack(P, axis=2)
    if inside.any():
        x = value(vol, [p[inside] for p in P], plane, samples, reduce)
        if table is None:
            table, domain = GREY_RAMP, (0.0, 1.0)
        T64 = np.ascontiguousarray(table, np.float32).astype(np.float64)
        n = T64.shape[0]
        dlo, dhi = float(f32(domain[0])), float(f32(domain[1]))
        k1 = f32((n - 1.0) / ((dhi - dlo) * SCALE[vol.dtype]))
        k2 = f32(-dlo * (n - 1.0) / (dhi - dlo))
        u = fma(x, k1, k2)
        U = np.fmin(np.where(u > f32(0.0), u, f32(0.0)), f32(n - 1)).astype(np.float64)  # a NaN and anything <= 0: entry 0
        i = np.minimum(np.floor(U).astype(np.int64), n - 2)
        f = U - i
        rgb[inside] = np.stack([srgb64(T64[i, k] + f * (T64[i + 1, k] - T64[i, k])) for k in range(3)], axis=1)
        val[inside, 0] = x
        val[inside, 1] = 1.0
    return rgb, val, pos, inside
