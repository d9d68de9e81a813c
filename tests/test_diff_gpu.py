"""vk_steady_diffusion on the MI355X, in use: VK_DIFF_INSTALL followed by the passes that read the field --
vk_volume_histogram gives exactly what the restatement's dense array predicts, and a table render of it stays finite; an install leaves
table, projection, isosurface, lighting and clip box in force; the Python wrapper with its derived values; the C++ host's
bonsai --diffusion on the fixed case."""
import math
import os
import subprocess

import numpy as np
import pytest

import diff_cases as DFC
import diff_helpers as DH
import dist_cases as DC
import geo_cases as GC
import label_helpers as LH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID = -1
W, H = 64, 64
PINNED = dict(n_foreground=206, n_inlet=21, n_outlet=21, n_box=252, sweeps=96, converged=1, Fin_q=328591872, Fout_q=328737975, sum_c_q=101749242837)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return DH.build_restatement(tmp_path_factory.mktemp("diff_gpu"))


def _ctx(V):  # noqa: F811
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    return V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)


def _table(V):  # noqa: F811
    return V.transfer_table([(0.0, 0.0, 0.0, 0.0, 0.0), (0.3, 0.1, 0.2, 0.9, 0.0), (0.5, 1.0, 0.5, 0.1, 0.4), (1.0, 1.0, 1.0, 1.0, 0.9)], 64)


def _frame(V, ctx):  # noqa: F811
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)
    return ctx.read_backbuffer().copy()


def _held(ctx):
    """The volume the context holds, as a dense array."""
    return ctx.keep_components(-math.inf, math.inf, keep="all", install=False, out=True)[0]


def _fixed(kind="u8"):
    return DC.mask_volume(GC.fixed_mask(), kind)


def _restate_fixed(lib, kind, **kw):
    args = dict(lo=0.5, hi=math.inf, axis=0, spacing=(1, 1, 1), omega=DFC.auto_omega(12), check_every=32, max_sweeps=20000, delta_tol=1e-5, flux_tol=1e-3)
    args.update(kw)
    return DH.restate(lib, _fixed(kind), kind, **args)


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED"), ("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_install_then_histogram_and_a_table_render_read_the_concentration_field(V, lib, kind, layout):  # noqa: F811
    """The fixed case along x at the defaults: the installed field is the restatement's dense array bit for bit, its histogram is that of
    a fresh upload of that array, and the table march renders it to finite pixels."""
    vol = _fixed(kind)
    c, dense, result = _restate_fixed(lib, kind)
    assert {k: DH.signed(result[DH.R[k]]) for k in PINNED} == PINNED
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
        info = ctx._volume_dtype()
        t = ctx.steady_diffusion(0.5, axis="x", install=True, out=True, c=True)
        assert DH.differences((t.c, t.dense, DH.result_array(t)), (c, dense, result)) == ""
        assert t.converged and t.sweeps == 96 and t.porosity == 206 / 252 and t.effective_diffusivity == t.flux * 12 / 21 and t.flux_mismatch < 1e-3 and ctx._volume_dtype() == info
        assert t.tortuosity_factor == t.porosity / t.effective_diffusivity and 4.0 < t.tortuosity_factor < 5.0 and t.extent == (12, 7, 3)
        assert (LH.raw(_held(ctx)) == LH.raw(dense)).all()                                          # ... and it was installed
        fresh = _ctx(V)
        try:
            LH.upload(V, fresh, dense, kind, layout)
            fresh.update()
            want = np.asarray(fresh.volume_histogram(64, (0.0, 1.0)).counts)
        finally:
            fresh.close()
        counts = np.asarray(ctx.volume_histogram(64, (0.0, 1.0)).counts)
        assert (counts == want).all() and int(counts.sum()) == vol.size and int(counts[0]) >= vol.size - 206 and int((counts > 0).sum()) > 20   # a graded field
        ctx.set_transfer_function(_table(V), (0.0, 1.0))
        frame = _frame(V, ctx)
        assert np.isfinite(frame).all() and np.abs(frame[..., :3]).sum() > 0
    finally:
        ctx.close()


STATES = {
    "table, lighting, clip box": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_lighting((0.3, 0.5, 0.8)), c.set_clip_box((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))),
    "table, max projection": lambda V, c: (c.set_transfer_function(_table(V), (0.0, 1.0)), c.set_projection("max")),
    "isosurface": lambda V, c: c.set_isosurface(0.35, (0.9, 0.8, 0.7), 4),
}


@pytest.mark.parametrize("state", sorted(STATES))
def test_an_install_leaves_table_projection_isosurface_lighting_and_clip_box_in_force(V, lib, state):  # noqa: F811
    """Context a installs the field under the state; context b gets the same state and a fresh upload of the restatement's field: the two
    render the same frame bit for bit, which they would not if the install had dropped any of the state."""
    c = next(c for c in DFC.cases() if c.kind == "u8" and "density 0.9" in c.name and c.box is None)
    dense = DH.restate_case(lib, c)[1]
    a, b = _ctx(V), _ctx(V)
    try:
        for ctx in (a, b):
            STATES[state](V, ctx)
        in_force = (a.isosurface, a.clip_box, a.projection)
        LH.upload(V, a, c.vol, "u8", "PACKED")
        LH.upload(V, b, dense, "u8", "PACKED")
        a.update()
        b.update()
        before = _frame(V, a)
        t = a.steady_diffusion(c.lo, c.hi, axis=c.axis, spacing=c.spacing, omega=c.omega, check_every=c.check_every, delta_tol=c.delta_tol, flux_tol=c.flux_tol, max_sweeps=c.max_sweeps,
                               install=True)
        assert t.n_foreground > 0 and t.dense is None and t.c is None
        assert (a.isosurface, a.clip_box, a.projection) == in_force == (b.isosurface, b.clip_box, b.projection)
        fa, fb = _frame(V, a), _frame(V, b)
        assert (fa.view(np.uint32) == fb.view(np.uint32)).all() and np.isfinite(fa).all() and np.abs(fa[..., :3]).sum() > 0
        assert not (fa.view(np.uint32) == before.view(np.uint32)).all()                             # the field is not the volume it came from
        assert (_held(a) == dense).all()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind, layout", [("u8", "PACKED_PAIRS"), ("u16", "LINEAR"), ("f16", "PACKED")])
def test_python_wrapper_against_the_restatement(V, lib, kind, layout):  # noqa: F811
    import label_cases as LC

    d = (33, 9, 10)
    vol = LC.noise(d, kind, 12)
    ctx = _ctx(V)
    try:
        LH.upload(V, ctx, vol, kind, layout)
        ctx.update()
        info = ctx._volume_dtype()
        want = DH.restate(lib, vol, kind, 0.3, math.inf, 2, (1, 1, 1), DFC.auto_omega(10), 32, 64, 1e-5, 1e-3)
        t = ctx.steady_diffusion(0.3, max_sweeps=64, out=True, c=True)                               # the defaults: along z, spacing 1, automatic omega, blocks of 32, no install
        assert t.c.dtype == np.float32 and t.dense.dtype == vol.dtype and DH.differences((t.c, t.dense, DH.result_array(t)), want) == ""
        assert t.omega == DFC.auto_omega(10) and t.gain == 1.0 and t.extent == d and t.axis == 2 and np.isnan(t.c).sum() == vol.size - t.n_foreground
        assert (LH.raw(_held(ctx)) == LH.raw(np.ascontiguousarray(vol))).all() and ctx._volume_dtype() == info   # not installed
        totals = ctx.steady_diffusion(0.3, max_sweeps=64)
        assert totals.c is None and totals.dense is None and (DH.result_array(totals) == want[2]).all()
        box = ((2, 1, 0), (30, 9, 7))
        want = DH.restate(lib, vol, kind, 0.2, 0.8, 1, (1, 2, 3), 1.5, 4, 40, 1e-4, 1e-2, 0.5, 0.25, box[0] + box[1])
        t = ctx.steady_diffusion(0.2, 0.8, axis="y", spacing=(1, 2, 3), omega=1.5, check_every=4, delta_tol=1e-4, flux_tol=1e-2, max_sweeps=40, gain=0.5, fill_out=0.25, box=box, out=True, c=True)
        assert DH.differences((t.c, t.dense, DH.result_array(t)), want) == "" and t.gain == 0.5 and t.extent == (28, 8, 7) and t.n_box == 28 * 8 * 7
        clip = ((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))
        ctx.set_clip_box(*clip)
        t = ctx.steady_diffusion(0.3, axis=0, box="clip", max_sweeps=64, c=True)
        ctx.set_clip_box(None)
        cb = LC.clip_voxel_box(clip[0], clip[1], d)
        want = DH.restate(lib, vol, kind, 0.3, math.inf, 0, (1, 1, 1), DFC.auto_omega(cb[3] - cb[0]), 32, 64, 1e-5, 1e-3, box=cb)
        assert DH.differences((t.c, None, DH.result_array(t)), (want[0], None, want[2])) == "" and t.extent == (cb[3] - cb[0], cb[4] - cb[1], cb[5] - cb[2])
        want = DH.restate(lib, vol, kind, 0.3, math.inf, 1, (2, 1, 1), DFC.auto_omega(9), 32, 64, 1e-5, 1e-3, 0.75)
        t = ctx.steady_diffusion(0.3, axis="y", spacing=(2, 1, 1), max_sweeps=64, gain=0.75, install=True)
        assert (DH.result_array(t) == want[2]).all() and (LH.raw(_held(ctx)) == LH.raw(want[1])).all() and ctx._volume_dtype() == info
        for bad in (dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(axis="q"), dict(omega=2.0), dict(check_every=0), dict(max_sweeps=8), dict(delta_tol=-1.0), dict(gain=math.inf)):
            with pytest.raises(ValueError):
                ctx.steady_diffusion(0.3, **bad)
        with pytest.raises(V.VokselisError) as e:
            ctx.steady_diffusion(0.6, 0.5)
        assert e.value.code == INVALID and "lo > hi" in str(e.value)
        with pytest.raises(V.VokselisError) as e:
            ctx.steady_diffusion(0.3, box=((0, 0, 0), (34, 9, 10)))
        assert e.value.code == INVALID and "leaves the volume" in str(e.value)
    finally:
        ctx.close()


def _bonsai():
    import __graft_entry__ as g

    g.build_host()
    return os.path.join(LH.ROOT, "vokselis_amd", "_lib", "bonsai")


def _line(t, spacing="1 1 1"):
    return ("diffusion: [0.5, inf] along x spacing %s: %d foreground voxels, porosity %.6g, %d sweeps, converged %s, flux in %.6g out %.6g, D_eff/D0 %.6g, tortuosity factor %.6g"
            % (spacing, t.n_foreground, t.porosity, t.sweeps, "yes" if t.converged else "no", t.flux_in, t.flux_out, t.effective_diffusivity, t.tortuosity_factor))


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_bonsai_diffusion_prints_the_fixed_case_and_installs_the_restatements_field(V, lib, tmp_path, kind):  # noqa: F811
    """bonsai --diffusion x on the fixed case prints the restatement's numbers; with --diffusion-install and --save-raw the saved file is
    the restatement's dense array, bit for bit."""
    import vokselis_amd

    vol = _fixed(kind)
    src, dst = tmp_path / "in.raw", tmp_path / "out.raw"
    vol.tofile(src)
    base = [_bonsai(), "--raw-u16" if kind == "u16" else "--raw", str(src), "--dims", "12", "7", "3", "--components", "0.5", "inf", "6", "--histogram", "4"]
    want = _restate_fixed(lib, kind)
    res = vokselis_amd.VkDiffusionResult(*[DH.signed(v) for v in want[2][:9]], 0.0, 0.0, 1.0, 0)
    t = vokselis_amd.Diffusion(res, 0, (12, 7, 3))
    r = subprocess.run(base + ["--diffusion", "x"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    assert _line(t) in r.stdout.splitlines(), r.stdout[-800:]
    r = subprocess.run(base + ["--diffusion", "x", "64", "--diffusion-install", "--label-fill", "0.25", "--save-raw", str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    want = _restate_fixed(lib, kind, max_sweeps=64, fill_out=0.25)
    t = vokselis_amd.Diffusion(vokselis_amd.VkDiffusionResult(*[DH.signed(v) for v in want[2][:9]], 0.0, 0.0, 1.0, 0), 0, (12, 7, 3))
    assert not t.converged and t.sweeps == 64 and _line(t) in r.stdout.splitlines(), r.stdout[-800:]
    got = np.fromfile(dst, vol.dtype).reshape(vol.shape)
    assert DH.differences((None, got, None), (None, want[1], None)) == ""
