"""An independent reference for light-direction shadows under a first-hit isosurface (vk_set_shadows), written from DESIGN.md section 17
and include/vokselis_hip.h, not from tests/shadow_restatement.c: vectorised numpy on top of tests/np_iso_reference.py.

The primary march, the bisection and the gradient are np_iso_reference's.  That reference reaches its refinement position through the module
attribute _back and its shade through the module attribute _shade, both looked up at call time; shadows() substitutes versions that
remember the shaded position q and shade with the shadow factor, for the duration of one call, and restores the originals after (the
way np_clip_reference.clip_box and np_u16_reference.u16 compose: no reference is edited, and both compose with this one -- the shadow
ray takes its box from oracle.np_restatement.intersect_box and its threshold from np_iso_reference.iso_k at call time).

What decides a shadow ray's fate is exact in f32: the step dts, intersect_box, ts0, the positions ps = fma(ts0, L, q) and ps + ss, the
loop variable t, and the hit test x >= iso_k per sample.  What only moves colour is float64: k = 1 - strength and
rgb' = c (ka + kd diff k) + ks spec k, which is linear in (ka, kd, ks): the unshadowed shade of (ka, 0, 0) plus k times that of (0, kd, ks)."""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import np_restatement as R

import np_iso_reference as NI
import np_u16_reference as NU
from np_clip_reference import clip_box
from np_table_reference import light_dir

f32 = np.float32


def cast(vol, q, direction, dt_scale, k_iso, bias):
    """The shadow rays of the points q (three f32 arrays) towards the light: (shadowed bool, iterations u32), exact in f32."""
    nz, ny, nx = vol.shape
    n = q[0].size
    Lf = [f32(v) for v in light_dir(direction)]
    Ld = [np.full(n, Lf[c], np.float32) for c in range(3)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dtv = [f32(1.0) / (f32(d) * np.abs(Lf[c])) for c, d in enumerate((nx, ny, nz))]
        dts = f32(f32(dt_scale) * np.fmin(dtv[0], np.fmin(dtv[1], dtv[2])))
        tb0, tb1 = R.intersect_box(q, Ld, 0.0, 1.0)
        ok = ~(tb0 > tb1)
        ts0 = np.fmax(np.fmax(tb0, f32(0.0)), f32(f32(bias) * dts)).astype(np.float32)
        ps = [R.fma(ts0, Ld[c], q[c]) for c in range(3)]
        ss = [f32(Lf[c] * dts) for c in range(3)]
        t = ts0.copy()
        shadowed = np.zeros(n, bool)
        iters = np.zeros(n, np.uint32)
        active = ok & (t < tb1)
        while active.any():
            idx = np.nonzero(active)[0]
            x = R.sample_trilinear(vol, [ps[c][idx] for c in range(3)], raw=True, taps=True)[0]
            iters[idx] += 1
            h = x >= k_iso
            shadowed[idx[h]] = True
            cont = idx[~h]
            for c in range(3):
                ps[c][cont] = (ps[c][cont] + ss[c]).astype(np.float32)
            t[cont] = (t[cont] + dts).astype(np.float32)
            active[idx[h]] = False
            active[cont] = t[cont] < tb1[cont]
    return shadowed, iters


@contextlib.contextmanager
def shadows(vol, dt_scale, iso, strength, bias, record):
    """While active, np_iso_reference shades with shadows; `record` receives "shadowed" and "iters" over the rays that hit, in ray order."""
    back, shade = NI._back, NI._shade
    seen = []

    def remember(m, s, p):
        q = back(m, s, p)
        seen.append(q)
        return q

    def shade_k(rgb, g, Ld, Hd, light):
        q = seen[-3:]  # the last three positions computed: q = fma(-a, s, p) of the rays that hit
        dark, it = cast(vol, q, light["direction"], dt_scale, NI.iso_k(iso, vol.dtype == np.uint8), bias)
        record["shadowed"], record["iters"] = dark, it
        k = np.where(dark, 1.0 - float(f32(strength)), 1.0)
        amb = shade(rgb, g, Ld, Hd, dict(light, diffuse=0.0, specular=0.0))
        rest = shade(rgb, g, Ld, Hd, dict(light, ambient=0.0))
        return [a + k * b for a, b in zip(amb, rest)]

    NI._back, NI._shade = remember, shade_k
    try:
        yield
    finally:
        NI._back, NI._shade = back, shade


def render(camera_blob: bytes, vol: np.ndarray, W: int, H: int, *, iso, colour=(1.0, 1.0, 1.0), refine=4, dt=1.0, light=None, shadow=None, box=None,
           tile=None):
    """(rgb float64 [H, W, 3], steps u32, nonempty u32, hit bool, a f32, shadowed bool, shadow iterations u32: each [H, W]).  vol: u8, f16
    or uint16 (R16_UNORM) [nz, ny, nx]; light: the keyword arguments of Context.set_lighting; shadow: (strength, bias) or None; box:
    (lo3, hi3) or None.  Shadows take effect with a light that is not a headlight, and are ignored otherwise."""
    vol = np.ascontiguousarray(vol)
    on = shadow is not None and light is not None and not isinstance(light["direction"], str)
    rec = {}
    with contextlib.ExitStack() as st:
        if vol.dtype == np.uint16:
            st.enter_context(NU.u16())
        st.enter_context(clip_box(box))
        if on:
            st.enter_context(shadows(vol, dt, iso, shadow[0], shadow[1], rec))
        rgb, steps, live, hit, a = NI.render(camera_blob, vol, W, H, iso=iso, colour=colour, refine=refine, dt=dt, light=light, tile=tile)
    dark = np.zeros((H, W), bool)
    iters = np.zeros((H, W), np.uint32)
    if on and "shadowed" in rec:  # (rays that hit are shaded in row-major order of the frame)
        dark[hit] = rec["shadowed"]
        iters[hit] = rec["iters"]
    return rgb, steps, live, hit, a, dark, iters
