"""Shared by the histogram tests: the C restatement (tests/hist_restatement.c, built with -ffp-contract=off), a case through it, and the
comparison of a result -- the library's, the restatement's or the numpy reference's -- with another."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np

import np_hist_reference as NH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"u8": 0, "f16": 1, "u16": 3}
KINDS = ("nan", "below", "above", "at_lo", "at_hi", "top_clamped", "neg_zero")  # hist_restatement.c's kind counters


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libhist_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "hist_restatement.c"), "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.hist_restate.restype = C.c_int
    return L


def restate(L, vol, kind, bins, domain, box=None, kinds=None):
    """The restatement's result as a dict like np_hist_reference.histogram's, its sums as the f64 it accumulated; kinds (a uint64 array of
    len(KINDS)) is added to."""
    v = np.ascontiguousarray(vol)
    raw = v.view(np.uint16) if kind == "f16" else v
    nz, ny, nx = v.shape
    (x0, y0, z0), (x1, y1, z1) = ((0, 0, 0), (nx, ny, nz)) if box is None else box
    b = np.array([x0, y0, z0, x1, y1, z1], np.uint32)
    lo_k, hi_k, k1, k2 = NH.constants(kind, domain[0], domain[1], bins)
    counts, cats, sums, mm = np.zeros(bins, np.uint64), np.zeros(4, np.uint64), np.zeros(2, np.float64), np.zeros(2, np.float32)
    kinds = np.zeros(len(KINDS), np.uint64) if kinds is None else kinds
    rc = L.hist_restate(C.c_void_p(raw.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(FMT[kind]), C.c_void_p(b.ctypes.data),
                        C.c_float(lo_k), C.c_float(hi_k), C.c_float(k1), C.c_float(k2), C.c_uint32(bins), C.c_void_p(counts.ctypes.data),
                        C.c_void_p(cats.ctypes.data), C.c_void_p(sums.ctypes.data), C.c_void_p(mm.ctypes.data), C.c_void_p(kinds.ctypes.data))
    assert rc == 0, rc
    return dict(counts=counts, n_voxels=(x1 - x0) * (y1 - y0) * (z1 - z0), n_nan=int(cats[0]), n_below=int(cats[1]), n_above=int(cats[2]), n_finite=int(cats[3]),
                min=mm[0], max=mm[1], sum=float(sums[0]), sum_sq=float(sums[1]))


def restate_case(L, c, kinds=None):
    return restate(L, c.vol, c.kind, c.bins, c.domain, c.box, kinds)


def from_histogram(h):
    """A vokselis_amd.Histogram as the same dict (on the kernel's scale)."""
    s = h.stats
    return dict(counts=h.counts, n_voxels=h.n_voxels, n_nan=h.n_nan, n_below=h.n_below, n_above=h.n_above, n_finite=h.n_finite,
                min=np.float32(s.min), max=np.float32(s.max), sum=float(s.sum), sum_sq=float(s.sum_sq))


def bits(x):
    return int(np.float32(x).view(np.uint32))


def integer_part_differences(got, ref):
    """What differs between two results in the parts that are integers or selections: counts, categories, min and max bit for bit."""
    out = []
    if got["counts"].shape != ref["counts"].shape or not (got["counts"] == ref["counts"]).all():
        out.append(f"counts differ in {int((got['counts'] != ref['counts']).sum()) if got['counts'].shape == ref['counts'].shape else 'shape'} bins")
    for k in ("n_voxels", "n_nan", "n_below", "n_above", "n_finite"):
        if int(got[k]) != int(ref[k]):
            out.append(f"{k} {int(got[k])} != {int(ref[k])}")
    for k in ("min", "max"):
        if bits(got[k]) != bits(ref[k]):
            out.append(f"{k} {got[k]!r} ({bits(got[k]):#010x}) != {ref[k]!r} ({bits(ref[k]):#010x})")
    if int(got["n_voxels"]) != int(got["n_nan"]) + int(got["n_below"]) + int(got["n_above"]) + int(got["counts"].sum()):
        out.append("n_voxels is not n_nan + n_below + n_above + sum(counts)")
    return out


def sum_differences(got, exact, kind):
    """The f64 sums of a result against the exact ones (np_hist_reference.histogram): equal for the integer formats, within
    (n - 1) 2^-53 sum|x| for f16 (sum_sq: its terms are its own absolute values)."""
    out = []
    n = int(exact["n_finite"])
    for k, a in (("sum", exact["abs_sum"]), ("sum_sq", exact["sum_sq"])):
        err = NH.sum_error(got[k], exact[k])
        bound = Fraction(0) if kind != "f16" else NH.sum_bound(n, a)
        if err > bound:
            out.append(f"{k} {got[k]!r} is {float(err):.3g} from the exact {float(exact[k])!r}, allowed {float(bound):.3g}")
    return out


LAYOUTS = {"u8": ("LINEAR", "PACKED", "PACKED_PAIRS"), "f16": ("LINEAR", "PACKED"), "u16": ("LINEAR", "PACKED")}


def upload(V, ctx, vol, kind, layout):
    kw = dict(fmt=V.FMT_R16_UNORM) if kind == "u16" else {}
    return V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout), **kw)

