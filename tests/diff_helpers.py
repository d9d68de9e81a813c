"""Shared by the steady-diffusion tests: the C restatement (tests/diff_restatement.c), a case through it and through the numpy reference,
the comparison of two results, a float64 direct solve of a case's linear system, and a case as the library's request.  Layouts and
uploads are the label tests' (label_helpers)."""
import ctypes as C
import os
import subprocess

import numpy as np

import diff_cases as DFC
import label_helpers as LH
import np_diff_reference as ND
import np_label_reference as NL

ROOT = LH.ROOT
RESULT = ("n_foreground", "n_inlet", "n_outlet", "n_box", "Fin_q", "Fout_q", "sum_c_q", "sweeps", "converged")
R = {k: i for i, k in enumerate(RESULT + ("delta", "omega", "gain"))}


def build_restatement(out_dir):
    so = os.path.join(str(out_dir), "libdiff_restatement.so")
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "diff_restatement.c"), "-lm"], check=True)
    L = C.CDLL(so)
    L.diff_restate.restype = C.c_int
    return L


def restate(L, vol, kind, lo, hi, axis, spacing, omega, check_every, max_sweeps, delta_tol, flux_tol, gain=0.0, fill_out=0.0, box=None):
    """(c float32 [nz, ny, nx], dense, result uint64 [12]: RESULT and the bits of delta, omega and the gain used)."""
    v = np.ascontiguousarray(vol)
    nz, ny, nx = v.shape
    b = np.array(box if box is not None else LH.whole(v), np.uint32)
    sp = np.array(spacing, np.uint32)
    c, dense, result = np.zeros(v.shape, np.float32), np.zeros_like(v), np.zeros(12, np.uint64)
    rc = L.diff_restate(C.c_void_p(v.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz), C.c_int(LH.FMT[kind]), C.c_float(lo), C.c_float(hi), C.c_uint32(axis),
                        C.c_void_p(sp.ctypes.data), C.c_float(omega), C.c_uint32(check_every), C.c_uint32(max_sweeps), C.c_float(delta_tol), C.c_float(flux_tol), C.c_float(gain),
                        C.c_float(fill_out), C.c_void_p(b.ctypes.data), C.c_void_p(c.ctypes.data), C.c_void_p(dense.ctypes.data), C.c_void_p(result.ctypes.data))
    assert rc == 0, rc
    return c, dense, result


def restate_case(L, c):
    return restate(L, c.vol, c.kind, c.lo, c.hi, c.axis, c.spacing, DFC.omega_used(c), c.check_every, c.max_sweeps, c.delta_tol, c.flux_tol, c.gain, c.fill_out, c.box)


def reference_case(c):
    return ND.apply(c.vol, c.kind, c.lo, c.hi, c.axis, c.spacing, DFC.omega_used(c), c.check_every, c.max_sweeps, c.delta_tol, c.flux_tol, c.gain, c.fill_out, c.box)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else LH.raw(a)


def differences(got, ref):
    """Where two results (c, dense, result) differ, in words (empty: bitwise equal)."""
    out = []
    for name, g, r in zip(("c", "dense", "result"), got, ref):
        if (g is None) != (r is None):
            out.append(f"{name}: present in one result only")
            continue
        if g is None:
            continue
        g, r = bits(g), bits(r)
        if g.shape != r.shape or g.dtype != r.dtype:
            out.append(f"{name}: shape / dtype {g.shape} {g.dtype} != {r.shape} {r.dtype}")
        elif (g != r).any():
            at = np.argwhere(g != r)[0]
            out.append(f"{name}: {int((g != r).sum())} of {g.size} differ, first at {tuple(int(v) for v in at)} (array order): {g[tuple(at)]} != {r[tuple(at)]}")
    return "; ".join(out)


def signed(v):
    v = int(v)
    return v - (1 << 64) if v >= 1 << 63 else v


def flux(result):
    return (signed(result[R["Fin_q"]]) + signed(result[R["Fout_q"]])) / 2147483648.0


def derived(c, result):
    """(porosity, D_eff / D0) of a case from a reference's result."""
    e = DFC.extent(c)
    cross = e[(c.axis + 1) % 3] * e[(c.axis + 2) % 3]
    return int(result[0]) / int(result[3]) if int(result[3]) else 0.0, flux(result) * e[c.axis] / cross if cross else 0.0


def direct_solve(c):
    """The case's linear system in float64, solved directly: (c64 [nz, ny, nx] with NaN where there is no equation, flux_in, flux_out).
    A voxel with den == 0 and the components of S that touch neither face (pure-Neumann, singular) are left out."""
    v = np.asarray(c.vol)
    nz, ny, nx = v.shape
    s = NL.foreground(v, c.kind, c.lo, c.hi, c.box)
    x0, y0, z0, x1, y1, z1 = c.box if c.box is not None else (0, 0, 0, nx, ny, nz)
    first, last = (x0, y0, z0)[c.axis], (x1, y1, z1)[c.axis] - 1
    # the components of S over the six neighbours, and which of them touch a face
    lab = NL.first_of_component(s, 6)
    along = np.indices(v.shape)[2 - c.axis]
    touching = set(np.unique(lab[s & ((along == first) | (along == last))]).tolist())
    keep = s & np.isin(lab, list(touching))
    idx = -np.ones(v.shape, np.int64)
    idx[keep] = np.arange(int(keep.sum()))
    n = int(keep.sum())
    w = [1.0 / float(c.spacing[k] ** 2) for k in range(3)]
    g = 2.0 * w[c.axis]
    A, b = np.zeros((n, n)), np.zeros(n)
    for z, y, x in np.argwhere(keep):
        i = idx[z, y, x]
        for k, (dz, dy, dx) in enumerate(((0, 0, 1), (0, 1, 0), (1, 0, 0))):
            for side in (-1, 1):
                uz, uy, ux = z + side * dz, y + side * dy, x + side * dx
                if 0 <= uz < nz and 0 <= uy < ny and 0 <= ux < nx and keep[uz, uy, ux]:
                    A[i, i] += w[k]
                    A[i, idx[uz, uy, ux]] -= w[k]
        a = (x, y, z)[c.axis]
        if a == first:
            A[i, i] += g
            b[i] += g
        if a == last:
            A[i, i] += g
    sol = np.linalg.solve(A, b) if n else np.zeros(0)
    c64 = np.full(v.shape, np.nan)
    c64[keep] = sol
    fin = float((2.0 * (1.0 - c64[keep & (along == first)])).sum())
    fout = float((2.0 * c64[keep & (along == last)]).sum())
    return c64, fin, fout


def request(c, install=False):
    """A case as the library's request (with VK_DIFF_CLIP_BOX where the case's box is the clip box) and its box argument."""
    from vokselis_amd import _native as N
    from vokselis_amd.diffusion import diffusion_request

    req = diffusion_request(c.lo, c.hi, axis=c.axis, spacing=c.spacing, omega=c.omega, check_every=c.check_every, delta_tol=c.delta_tol, flux_tol=c.flux_tol, max_sweeps=c.max_sweeps,
                            gain=c.gain, fill_out=c.fill_out, box="clip" if c.clip is not None else None, install=install)
    vb = N.VkVoxelBox(*c.box) if c.box is not None and c.clip is None else None
    return req, vb


def result_array(res):
    f = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
    return np.array([int(getattr(res, k)) & 0xFFFFFFFFFFFFFFFF for k in RESULT] + [f(res.delta), f(res.omega), f(res.gain)], np.uint64)


def fresh_result(N):
    return N.VkDiffusionResult(7, 7, 7, 7, 7, 7, 7, 7, 7, 7.0, 7.0, 7.0, 7)


def run(V, ctx, c, install=False, want_c=True, dense=True):
    """vk_steady_diffusion of a case: (rc, (c or None, dense or None, result)).  Outputs start from a pattern the call must overwrite."""
    N = V.native
    req, vb = request(c, install)
    arr = np.full(c.vol.shape, 0xABABABAB, np.uint32).view(np.float32) if want_c else None
    out = np.full_like(np.ascontiguousarray(c.vol), 0x5A if c.kind == "u8" else 0) if dense else None
    res = fresh_result(N)
    rc = N.lib().vk_steady_diffusion(ctx.handle, C.byref(req), C.byref(vb) if vb is not None else None, arr.ctypes.data if arr is not None else None,
                                     out.ctypes.data if out is not None else None, C.byref(res))
    return rc, (arr, out, result_array(res))


assert DFC.MAX_VOXELS == 64000
