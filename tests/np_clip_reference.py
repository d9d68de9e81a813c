"""The numpy references of the table, MAX and isosurface marches under a clip box (vk_set_clip_box).

The three references (tests/np_table_reference.py, np_mip_reference.py, np_iso_reference.py) reach the box through
oracle.np_restatement.intersect_box, a module attribute looked up at call time inside naive_rays.  clip_box() substitutes a version with
the box's bounds per axis -- the same f32 operations, lo[i] and hi[i] for lo and hi -- for the duration of one call and restores the
original after; everything behind the intersection (the miss, t0 = max(t0, 0), dt, the loop, the family's epilogue) is the references'
own, as the header says of the kernels.  No reference is edited."""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import np_restatement as R

import np_iso_reference as NI
import np_mip_reference as NM
import np_table_reference as NT

f32 = np.float32
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def intersect_clip(o, d, lo3, hi3):
    """np_restatement.intersect_box with bounds per axis."""
    tmin, tmax = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(3):
            inv = (f32(1.0) / d[i]).astype(np.float32)
            a = ((f32(lo3[i]) - o[i]) * inv).astype(np.float32)
            b = ((f32(hi3[i]) - o[i]) * inv).astype(np.float32)
            tmin.append(np.fmin(a, b))
            tmax.append(np.fmax(a, b))
    t0 = np.fmax(tmin[0], np.fmax(tmin[1], tmin[2]))
    t1 = np.fmin(tmax[0], np.fmin(tmax[1], tmax[2]))
    return t0, t1


@contextlib.contextmanager
def clip_box(box):
    """While active, the NAIVE rays of oracle.np_restatement march `box` = (lo3, hi3); None: nothing is substituted."""
    if box is None:
        yield
        return
    lo3, hi3 = box
    original = R.intersect_box

    def per_axis(o, d, lo, hi):
        assert (lo, hi) == (0.0, 1.0), "only the NAIVE rays take a clip box"
        return intersect_clip(o, d, lo3, hi3)

    R.intersect_box = per_axis
    try:
        yield
    finally:
        R.intersect_box = original


def render_table(box, *args, **kw):
    """np_table_reference.render (table, and lit with light=...) under the box: (rgb, steps)."""
    with clip_box(box):
        return NT.render(*args, **kw)


def render_mip(box, *args, **kw):
    """np_mip_reference.render under the box: (rgb, steps, nonempty)."""
    with clip_box(box):
        return NM.render(*args, **kw)


def render_iso(box, *args, **kw):
    """np_iso_reference.render under the box: (rgb, steps, nonempty, hit, a)."""
    with clip_box(box):
        return NI.render(*args, **kw)


def ray_hits_f64(camera_blob: bytes, W: int, H: int, box=UNIT, margin=1e-6):
    """bool [H, W]: the float64 ray through the pixel's centre passes through the box in front of the eye, by `margin` in t (a grazing ray
    may go either way in f32, and either way its pixel is clear-coloured)."""
    cam = np.frombuffer(camera_blob, np.float32).astype(np.float64)
    eye, m = cam[0:3], cam[20:36].reshape(4, 4)  # m[c] is column c
    X, Y = np.meshgrid(2.0 * (np.arange(W) + 0.5) / W - 1.0, 1.0 - 2.0 * (np.arange(H) + 0.5) / H)
    q = m[0][:, None, None] * X + m[1][:, None, None] * Y + (m[2] + m[3])[:, None, None]
    t0 = np.full((H, W), -np.inf)
    t1 = np.full((H, W), np.inf)
    ok = np.ones((H, W), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(3):
            d = q[k] / q[3] - eye[k]
            ta, tb = (float(f32(box[0][k])) - eye[k]) / d, (float(f32(box[1][k])) - eye[k]) / d
            ok &= ~(np.isnan(ta) | np.isnan(tb))
            t0 = np.maximum(t0, np.fmin(ta, tb))
            t1 = np.minimum(t1, np.fmax(ta, tb))
    return ok & (t1 > np.maximum(t0, 0.0) + margin)
