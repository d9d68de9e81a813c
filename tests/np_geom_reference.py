"""An independent reference for the geometry pass of the first-hit isosurface (vk_render_geometry), written from DESIGN.md section 18 and
include/vokselis_hip.h, not from tests/geom_restatement.c: vectorised numpy on top of tests/np_iso_reference.py.

The march and the bisection are np_iso_reference's, run with a light so that it forms the shaded position q = fma(-a, s, p) and the
gradient there.  That reference reaches q through the module attribute _back and its shade through _shade, both looked up at call time;
geometry() substitutes versions that remember q and the gradient for the duration of one call and restores the originals after (the way
np_shadow_reference.shadows composes: no reference is edited, and np_u16_reference.u16 and np_clip_reference.clip_box compose with it).

Exact in f32: the hit mask, a, q, the distance t = fma(q.z - e.z, d.z, fma(q.y - e.y, d.y, (q.x - e.x) d.x)) and the filtered sample x at
q (oracle.np_restatement.sample_trilinear).  In float64, from the eight taps: the gradient g (np_table_reference._gradient)."""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import np_restatement as R

import np_iso_reference as NI
import np_u16_reference as NU
from np_clip_reference import clip_box

f32 = np.float32
_LIGHT = dict(direction=(0.0, 0.0, 1.0), ambient=1.0, diffuse=0.0, specular=0.0, shininess=1.0)  # any light: only q and g are taken


@contextlib.contextmanager
def geometry(record):
    """While active, np_iso_reference's shade records "q" (three f32 arrays) and "g" (three float64 arrays) over the rays that hit."""
    back, shade = NI._back, NI._shade
    seen = []

    def remember(m, s, p):
        q = back(m, s, p)
        seen.append(q)
        return q

    def keep(rgb, g, Ld, Hd, light):
        record["q"], record["g"] = seen[-3:], g  # the last three positions computed: q = fma(-a, s, p) of the rays that hit
        return rgb

    NI._back, NI._shade = remember, keep
    try:
        yield
    finally:
        NI._back, NI._shade = back, shade


def render(camera_blob: bytes, vol: np.ndarray, W: int, H: int, *, iso, refine=4, dt=1.0, box=None, tile=None):
    """(pos_t f32 [H, W, 4]: q and t, the miss record's (0, 0, 0, +inf) where no ray hit; g float64 [H, W, 3]; x f32 [H, W]; hit bool, a f32,
    steps u32: each [H, W]).  vol: u8, f16 or uint16 (R16_UNORM) [nz, ny, nx]; box: (lo3, hi3) or None.  Pixels outside `tile` hold the
    miss record too."""
    vol = np.ascontiguousarray(vol)
    nz, ny, nx = vol.shape
    rec = {}
    with contextlib.ExitStack() as st, np.errstate(invalid="ignore", over="ignore"):
        if vol.dtype == np.uint16:
            st.enter_context(NU.u16())
        st.enter_context(clip_box(box))
        st.enter_context(geometry(rec))
        _, steps, _, hit, a = NI.render(camera_blob, vol, W, H, iso=iso, refine=refine, dt=dt, light=_LIGHT, tile=tile)
        rays = R.naive_rays(camera_blob, (nx, ny, nz), W, H, dt, tile)
    pos_t = np.zeros((H, W, 4), np.float32)
    pos_t[..., 3] = np.inf
    g_out = np.zeros((H, W, 3), np.float64)
    x_out = np.zeros((H, W), np.float32)
    if hit.any():
        q, g = rec["q"], rec["g"]
        sel = hit[np.ix_(rays["ys"], rays["xs"])].ravel()  # (rays that hit are shaded in row-major order of the tile)
        eye = np.frombuffer(camera_blob, np.float32)[:3]
        d = [rays["d"][c][sel] for c in range(3)]
        with np.errstate(invalid="ignore", over="ignore"):
            e = [(q[c] - eye[c]).astype(np.float32) for c in range(3)]
            t = R.fma(e[2], d[2], R.fma(e[1], d[1], (e[0] * d[0]).astype(np.float32)))
            x = R.sample_trilinear(vol, q, raw=True, taps=True)[0]
        pos_t[hit] = np.stack([q[0], q[1], q[2], t], axis=1)
        g_out[hit] = np.stack([np.asarray(v, np.float64) for v in g], axis=1)
        x_out[hit] = x
    return pos_t, g_out, x_out, hit, a, steps
