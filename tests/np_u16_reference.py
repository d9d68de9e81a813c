"""The numpy references of the built-in, table, lit, MAX and isosurface marches on R16_UNORM volumes (VK_FMT_R16_UNORM; DESIGN.md
section 16).

The references (tests/np_builtin_reference.py, np_table_reference.py, np_mip_reference.py, np_iso_reference.py) know two scales: u8 taps
on 0..255 and f16 values.  A uint16 array passes through oracle.np_restatement.sample_trilinear(raw=True, taps=True) as integer taps
0..65535, exact in f32, filtered as every other format is; what is left of the format is the scale S = 65535 in four module attributes,
each looked up at call time:
    np_table_reference.tf_constants and np_mip_reference.tf_constants   k1 = (n-1) / ((hi-lo) 65535), k2 as it was
    np_iso_reference.iso_k                                               iso * 65535 in f32
    np_builtin_reference.transfer_alpha                                  c = 58981.5, k1 = f32(1 / (65535 * 1.1)), k2 = f32(-0.1 / 1.1)
    np_builtin_reference.tap_empty                                       t <= 6553
u16() substitutes them for the duration of one call and restores the originals after.  No reference is edited.  The clip box composes
through np_clip_reference.clip_box."""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import np_restatement as R

import np_builtin_reference as NB
import np_iso_reference as NI
import np_mip_reference as NM
import np_table_reference as NT
from np_clip_reference import clip_box

f32 = np.float32
S = 65535.0
EMPTY_MAX = 6553  # the largest tap the built-in transfer maps to alpha +0


def tf_constants(n, lo, hi, r8=False):
    lo, hi = float(f32(lo)), float(f32(hi))
    span, nm1 = hi - lo, float(n) - 1.0
    return f32(nm1 / (span * S)), f32(-lo * nm1 / span)


def iso_k(iso, r8=False):
    with np.errstate(over="ignore"):
        return f32(iso) * f32(S)


def transfer_alpha(x, r8=False):
    s = R.fma(np.fmin(np.asarray(x, np.float32), f32(58981.5)), f32(1.0 / (S * 1.1)), f32(-0.1 / 1.1))
    s = np.fmin(np.fmax(s, f32(0.0)), f32(1.0))
    return ((s * s).astype(np.float32) * R.fma(f32(-2.0), s, f32(3.0))).astype(np.float32)


def tap_empty(t, f16=False):
    return np.asarray(t, np.float32) <= f32(EMPTY_MAX)


@contextlib.contextmanager
def u16():
    """While active, the four references compute on the R16_UNORM scale."""
    saved = (NT.tf_constants, NM.tf_constants, NI.iso_k, NB.transfer_alpha, NB.tap_empty)
    NT.tf_constants, NM.tf_constants, NI.iso_k, NB.transfer_alpha, NB.tap_empty = tf_constants, tf_constants, iso_k, transfer_alpha, tap_empty
    try:
        yield
    finally:
        NT.tf_constants, NM.tf_constants, NI.iso_k, NB.transfer_alpha, NB.tap_empty = saved


def _vol(vol):
    vol = np.ascontiguousarray(vol)
    assert vol.dtype == np.uint16 and vol.ndim == 3, "an R16_UNORM volume is uint16 [nz, ny, nx]"
    return vol


def render_builtin(cam, vol, W, H, **kw):
    """np_builtin_reference.render on the u16 scale: (rgb, steps, sampled)."""
    with u16():
        return NB.render(cam, _vol(vol), W, H, **kw)


def render_table(box, cam, vol, W, H, **kw):
    """np_table_reference.render (table, and lit with light=...) on the u16 scale under the clip box (None: the unit cube): (rgb, steps)."""
    with u16(), clip_box(box):
        return NT.render(cam, _vol(vol), W, H, **kw)


def render_mip(box, cam, vol, W, H, **kw):
    """np_mip_reference.render: (rgb, steps, nonempty)."""
    with u16(), clip_box(box):
        return NM.render(cam, _vol(vol), W, H, **kw)


def render_iso(box, cam, vol, W, H, **kw):
    """np_iso_reference.render: (rgb, steps, nonempty, hit, a)."""
    with u16(), clip_box(box):
        return NI.render(cam, _vol(vol), W, H, **kw)


# ---- the census of a PACKED volume's cells under the predicate in force --------------------------------------------------------------

def cell_taps(vol):
    """The eight taps (f32) of every cell of the PACKED layout, padding cells included: physical brick B holds the cells of low-corner
    voxels 4 (B - 1) .. 4 (B - 1) + 3, so i runs over [-4, 4 nb - 5] per axis with nb = ((n - 1) >> 2) + 2 bricks, indices clamped to the
    volume.  Tap b = dx + 2 dy + 4 dz."""
    vol = _vol(vol)
    nz, ny, nx = vol.shape
    ax = []
    for n in (nx, ny, nz):
        i = np.arange(-4, 4 * (((n - 1) >> 2) + 2) - 4)
        ax.append((np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1)))
    taps = []
    for b in range(8):
        x, y, z = ax[0][b & 1], ax[1][(b >> 1) & 1], ax[2][b >> 2]
        taps.append(vol[np.ix_(z, y, x)].astype(np.float32))
    return taps


def empty_fraction(vol, *, table=None, domain=(0.0, 1.0), mip=False, iso=None):
    """vk_volume_empty_fraction of the PACKED layout: the share of cells empty under the isosurface's predicate (iso), the maximum
    projection's (mip; table None: the grey ramp), the table's, or the built-in one."""
    taps = cell_taps(vol)
    t = np.stack(taps)
    m, M = t.min(axis=0), t.max(axis=0)
    if iso is not None:
        e = M < iso_k(iso)
    elif mip:
        n = 2 if table is None else len(table)
        k1, k2 = tf_constants(n, *((0.0, 1.0) if table is None else domain))
        e = NM.tf_u(M, k1, k2, f32(n - 1)) == 0
    elif table is not None:
        T = np.ascontiguousarray(table, np.float32)
        n = len(T)
        k1, k2 = tf_constants(n, *domain)
        prefix = np.concatenate([[0], np.cumsum(T[:, 3] != 0)])
        lo = np.maximum(np.floor(NM.tf_u(m, k1, k2, f32(n - 1))).astype(np.int64) - 1, 0)
        hi = np.minimum(np.floor(NM.tf_u(M, k1, k2, f32(n - 1))).astype(np.int64) + 2, n - 1)
        e = prefix[hi + 1] == prefix[lo]
    else:
        e = M <= f32(EMPTY_MAX)
    return float(e.sum()) / float(e.size)
