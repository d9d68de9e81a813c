"""Shared by the measure tests: the C restatement (tests/measure_restatement.c), a case's labels (from the label restatement for a value
range, or the case's own), a case through both references, a case as the library's request, the call on a context, and vk_region records
as the uint64 [n, 27] table the references use.  Layouts and the upload are label_helpers'."""
import ctypes as C
import os
import subprocess

import numpy as np

import label_helpers as LH
import measure_cases as MC
import np_measure_reference as NM

ROOT = LH.ROOT
COLS = NM.COLS
ROOM = 8192  # records a call makes room for where the regions come from a value range: more than any case has
COLUMN_NAMES = ("n_voxels first x0 y0 z0 x1 y1 z1 sum_x sum_y sum_z sum_xx sum_yy sum_zz sum_xy sum_xz sum_yz n_nonfinite q_min q_max sum_q_hi sum_q_lo sum_qq_hi "
                "sum_qq_lo faces_x faces_y faces_z").split()
assert len(COLUMN_NAMES) == COLS


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libmeasure_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "measure_restatement.c"), "-lm"],
                   check=True)
    L = C.CDLL(so)
    L.measure_restate.restype = C.c_int
    return L


def restate(L, vol, kind, labels, n_regions):
    """(table uint64 [n_regions, 27], n_foreground); raises on a label above n_regions."""
    v, lab = np.ascontiguousarray(vol), np.ascontiguousarray(labels, np.uint32)
    nz, ny, nx = v.shape
    table, fg = np.zeros((max(int(n_regions), 1), COLS), np.uint64), C.c_uint64(0)
    rc = L.measure_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(LH.FMT[kind]), C.c_void_p(lab.ctypes.data), C.c_uint64(int(n_regions)),
                           C.c_void_p(table.ctypes.data), C.byref(fg))
    assert rc == 0, rc
    return table[:int(n_regions)].copy(), int(fg.value)


_LABELS = {}


def case_labels(label_lib, c):
    """(labels uint32 [nz, ny, nx], n_regions, label table or None) of a case: the label restatement's for a value range (computed once)."""
    if c.labels is not None:
        return c.labels, c.max_label, None
    if c.name not in _LABELS:
        labels, table, result, _ = LH.restate(label_lib, c.vol, c.kind, c.lo, c.hi, c.conn, c.box)
        labels.setflags(write=False)
        _LABELS[c.name] = (labels, int(result[0]), table)
    return _LABELS[c.name]


def restate_case(L, label_lib, c):
    labels, n, _ = case_labels(label_lib, c)
    return restate(L, c.vol, c.kind, labels, n)


def reference_case(label_lib, c):
    labels, n, _ = case_labels(label_lib, c)
    return NM.measure(c.vol, c.kind, labels, n)


def differences(got, ref):
    """Where two tables differ, in words (empty: bitwise equal)."""
    if got.shape != ref.shape:
        return f"shape {got.shape} != {ref.shape}"
    if (got == ref).all():
        return ""
    k, col = (int(v) for v in np.argwhere(got != ref)[0])
    return f"{int((got != ref).sum())} of {got.size} words differ, first in region {k + 1}, {COLUMN_NAMES[col]}: {int(got[k, col])} != {int(ref[k, col])}"


def request(c, labels_in=False):
    """A case as the library's request and its box argument.  labels_in: the regions come from a label array (the case's own, or -- for a
    value range -- one the caller obtained elsewhere), so range, connectivity and box stay 0; max_label is the caller's to fill in."""
    from vokselis_amd import _native as N
    from vokselis_amd.measure import measure_request

    if labels_in or c.labels is not None:
        return measure_request(max_label=max(c.max_label, 1)), None
    req = measure_request(c.lo, c.hi, connectivity=c.conn, box="clip" if c.clip is not None else None)
    vb = N.VkVoxelBox(*c.box) if c.box is not None and c.clip is None else None
    return req, vb


def table_array(regions, n):
    """n vk_region as the uint64 [n, 27] the references use (signed fields as their two's complement)."""
    from vokselis_amd.measure import REGION_DTYPE

    rec = np.frombuffer(regions, REGION_DTYPE, count=n) if n else np.zeros(0, REGION_DTYPE)
    out = np.zeros((n, COLS), np.uint64)
    out[:, 0], out[:, 1], out[:, 2:8], out[:, 8:17], out[:, 17] = rec["n_voxels"], rec["first"], rec["box"], rec["sums"], rec["n_nonfinite"]
    out[:, 18], out[:, 19], out[:, 20] = rec["q_min"].view(np.uint64), rec["q_max"].view(np.uint64), rec["sum_q_hi"].view(np.uint64)
    out[:, 21], out[:, 22], out[:, 23], out[:, 24:27] = rec["sum_q_lo"], rec["sum_qq_hi"], rec["sum_qq_lo"], rec["faces"]
    return out


def regions_from_table(table):
    """The uint64 [n, 27] table as n vk_region: table_array's inverse."""
    from vokselis_amd import _native as N
    from vokselis_amd.measure import REGION_DTYPE

    n = len(table)
    rec = np.zeros(max(n, 1), REGION_DTYPE)
    r = rec[:n]
    r["n_voxels"], r["first"], r["box"], r["sums"], r["n_nonfinite"] = table[:, 0], table[:, 1], table[:, 2:8], table[:, 8:17], table[:, 17]
    r["q_min"], r["q_max"], r["sum_q_hi"] = table[:, 18].view(np.int64), table[:, 19].view(np.int64), table[:, 20].view(np.int64)
    r["sum_q_lo"], r["sum_qq_hi"], r["sum_qq_lo"], r["faces"] = table[:, 21], table[:, 22], table[:, 23], table[:, 24:27]
    return (N.VkRegion * max(n, 1)).from_buffer_copy(rec.tobytes())


def run(V, ctx, c, labels=None, max_label=None, cap=None, want_regions=True, want_result=True):
    """vk_measure_components of a case: (rc, table uint64 [records_written, 27], VkMeasureResult).  labels: an array to pass as labels_in
    in place of the case's own source (with its max_label)."""
    N = V.native
    lab = labels if labels is not None else c.labels
    req, vb = request(c, labels_in=lab is not None)
    if lab is not None:
        lab = np.ascontiguousarray(lab, np.uint32)
        req.max_label = int(max_label if max_label is not None else c.max_label)
    room = (int(req.max_label) if lab is not None else min(c.vol.size, ROOM)) if cap is None else cap
    regions = (N.VkRegion * max(room, 1))()
    res = N.VkMeasureResult()
    rc = N.lib().vk_measure_components(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, lab.ctypes.data if lab is not None else None,
                                       regions if want_regions else None, room, C.byref(res) if want_result else None)
    return rc, table_array(regions, int(res.records_written) if rc == 0 and want_result else 0), res


assert MC.MAX_VOXELS == 64 * 64 * 33
