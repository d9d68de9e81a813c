"""Shared by the volume filter tests: the C restatement (tests/filter_restatement.c, built with -ffp-contract=off), a case through it, the
bitwise comparison of two dense volumes, and the layouts of each format with their upload."""
import ctypes as C
import os
import subprocess

import numpy as np

import filter_cases as FC
import np_filter_reference as NF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = {"u8": 0, "f16": 1, "u16": 3}
OPS = {"convolve": 0, "median3": 1}
KINDS = ("clamp x lo", "clamp x hi", "clamp y lo", "clamp y hi", "clamp z lo", "clamp z hi", "rint ties", "clamped low", "clamped high", "NaN out", "inf out", "median ties")


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libfilter_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "filter_restatement.c"), "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.filter_restate.restype = C.c_int
    return L


def restate(L, vol, kind, op, radii, weights, kinds=None):
    """The restatement's dense output [nz, ny, nx] in the volume's dtype; kinds (a uint64 array of len(KINDS)) is added to.  weights: a
    [3][13] float32 array, or three arrays / None."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    w = np.zeros((3, NF.TAPS), np.float32)
    for a in range(3):
        if weights is not None and weights[a] is not None:
            w[a, :len(weights[a])] = weights[a]
    r = np.array(radii, np.uint32)
    out = np.zeros_like(v)
    kinds = np.zeros(len(KINDS), np.uint64) if kinds is None else kinds
    rc = L.filter_restate(C.c_void_p(v.ctypes.data), C.c_void_p(out.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(FMT[kind]), C.c_int(OPS[op]),
                          C.c_void_p(r.ctypes.data), C.c_void_p(w.ctypes.data), C.c_void_p(kinds.ctypes.data))
    assert rc == 0, rc
    return out


def restate_case(L, c, kinds=None):
    return restate(L, c.vol, c.kind, c.op, c.radii, c.weights, kinds)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((raw(a) == raw(b)).all())


def differences(got, ref):
    """A short description of where two dense volumes differ (empty: bitwise equal)."""
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return f"shape / dtype {got.shape} {got.dtype} != {ref.shape} {ref.dtype}"
    bad = np.argwhere(raw(got) != raw(ref))
    if len(bad) == 0:
        return ""
    z, y, x = bad[0]
    return f"{len(bad)} of {got.size} voxels differ, first at (x, y, z) = ({x}, {y}, {z}): {raw(got)[z, y, x]:#x} != {raw(ref)[z, y, x]:#x}"


LAYOUTS = {"u8": ("LINEAR", "PACKED", "PACKED_PAIRS"), "f16": ("LINEAR", "PACKED"), "u16": ("LINEAR", "PACKED")}


def upload(V, ctx, vol, kind, layout):
    kw = dict(fmt=V.FMT_R16_UNORM) if kind == "u16" else {}
    return V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout), **kw)


def request(V, c, install=False):
    """A case as the library's request."""
    from vokselis_amd.filter import filter_request

    return filter_request(c.weights, c.op, install)


def filter_dense(V, ctx, req, vol):
    """vk_volume_filter with dense_out: the output in the dtype and shape of `vol`; returns (rc, out)."""
    from vokselis_amd import _native as N

    out = np.zeros_like(np.ascontiguousarray(vol))
    rc = N.lib().vk_volume_filter(ctx.handle, C.byref(req), C.c_void_p(out.ctypes.data))
    return rc, out


def tile_shapes_in_the_header():
    """kFilterTiles and kMedianTile as vokselis_amd/csrc/vk_filter.hpp states them."""
    import re

    src = open(os.path.join(ROOT, "vokselis_amd", "csrc", "vk_filter.hpp")).read()
    m = re.search(r"kFilterTiles\[kFilterClasses\] = \{(.*?)\};", src)
    tiles = tuple(tuple(int(v) for v in re.findall(r"(\d+)u", t)) for t in re.findall(r"\{([^{}]*)\}", m.group(1)))
    med = tuple(int(v) for v in re.findall(r"(\d+)u", re.search(r"kMedianTile = \{(.*?)\};", src).group(1)))
    return tiles, med


assert FC.MAX_VOXELS == 25000
