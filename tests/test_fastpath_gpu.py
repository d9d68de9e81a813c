"""The cell marches at, near and beyond the limits of the rule that picks their unclamped build, on the MI355X (the cases:
tests/fastpath_cases.py; what the CPU suite has settled about them: tests/test_fastpath_cpu.py -- among it that every case the rule calls
"fast" looks up nothing outside the index tables, and that the seven rows a distance-only rule would send down the unclamped build do).

For every case on every cell layout of its format (u8: PACKED, PACKED_PAIRS; f16 and R16_UNORM: PACKED), built-in transfer and table:
- vk_debug_march_path answers what fastpath_cases.rule_fast computes for the case, and "safe" under RENDER_SAFE;
- per-pixel step counts equal the reference's (the C oracle built-in, the table restatement under the table; for R16_UNORM, which those two
  do not have, the numpy references on the u16 scale) under every policy;
- colour within the family's bar (gpu_helpers.TOL built-in, TOL_UNLIT table), finite, alpha 1;
- the default policy, RENDER_FORCE_SKIP | RENDER_PROBE_ALWAYS, RENDER_NO_SKIP and RENDER_SAFE give equal bits and equal steps;
- the production kernel (no RENDER_COUNT) gives the COUNT kernel's frame bit for bit.
The lit table, the maximum projection, the isosurface, the isosurface with shadows and the geometry pass run the same checks on one
long-axis case and one far-camera case on each side of the rule, and on a long R16_UNORM ray the rule keeps unclamped, against their own
restatements (lit and MAX on R16_UNORM: the numpy references) and bars.  A batch of five cameras, one beyond the precision
limit, equals its singles frame by frame; the near singles report the unclamped build, the batch's farthest camera the clamped one."""
import time

import numpy as np
import pytest

import fastpath_cases as FC
import geom_helpers as GH
import lit_helpers
import mip_helpers as MH
import np_u16_reference as NU
import shadow_helpers as SH
from gpu_helpers import TOL, V  # noqa: F401
from test_fastpath_cpu import references, rel_err, tf_lib  # noqa: F401
from test_mip_fuzz_gpu import TOL as TOL_MIP
from test_table_fuzz_gpu import TOL_LIT, TOL_UNLIT

pytestmark = pytest.mark.gpu

ISO, REFINE, COLOUR = 28.5 / 255.0, 4, (0.9, 0.8, 0.3)      # between the slabs at 28 and 29: a ray from the front crosses 70 % of the long axis
LIGHT = dict(direction=(-1.0, 0.02, 0.01), ambient=0.25, diffuse=0.8, specular=0.4, shininess=24.0)   # back along the long x axis: long shadow rays
SHADOWS = (0.6, 2.0)


def _layouts(c):
    return ("PACKED", "PACKED_PAIRS") if c.kind == "u8" else ("PACKED",)


def _policies(V):
    # the first is the one held to the reference; the others must reproduce it bit for bit
    return (("default", 0), ("force+probe", V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS), ("no skip", V.RENDER_NO_SKIP), ("safe", V.RENDER_SAFE))


def _bits(a):
    return a.view(np.uint32)


def _render(V, ctx, c, flags):
    from vokselis_amd import _native as N

    N.check(ctx.handle, N.lib().vk_backbuffer_clear(ctx.handle))
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=c.dt, flags=flags).record(ctx)
    return ctx.read_backbuffer().copy(), (ctx.read_steps().copy() if flags & V.RENDER_COUNT else None)


def _context(V, O, c, layout, setup):
    ctx = V.Context(c.W, c.H, backbuffer=(c.W, c.H), out_format=V.OUT_RGBA32F)
    try:
        setup(ctx)
        V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout), **(dict(fmt=V.FMT_R16_UNORM) if c.u16 else {}))
        ctx.set_camera_blob(c.blob(O))
    except BaseException:
        ctx.close()
        raise
    return ctx


def _check_path(V, O, ctx, c, what, fails):
    want = FC.rule_fast(c.dims, FC.eye_of(O, c), c.dt, 16 if what[1] == "PACKED_PAIRS" else c.cell_bytes)
    got = ctx.march_path_fast(c.dt, 0)
    if got != want:
        fails.append((what, f"vk_debug_march_path says {'fast' if got else 'safe'}, the rule {'fast' if want else 'safe'}"))
    if ctx.march_path_fast(c.dt, V.RENDER_SAFE) or ctx.march_path_fast(c.dt, V.RENDER_SAFE | V.RENDER_NO_SKIP):
        fails.append((what, "vk_debug_march_path says fast under RENDER_SAFE"))
    return want


def _check_frames(V, ctx, c, what, ref, ref_steps, tol, fails, worst):
    """The policies against the reference and against each other; the production kernel against the COUNT kernel."""
    frames = [(name, *_render(V, ctx, c, fl | V.RENDER_COUNT)) for name, fl in _policies(V)]
    prod, _ = _render(V, ctx, c, 0)
    _, img, steps = frames[0]
    if not (steps == ref_steps).all():
        fails.append((what, f"steps differ from the reference at {int((steps != ref_steps).sum())} pixels (largest {int(steps.max())}, the reference's {int(ref_steps.max())})"))
    if not (np.isfinite(img).all() and (img[..., 3] == 1.0).all()):
        fails.append((what, "a non-finite colour or an alpha that is not 1"))
    err = float(rel_err(img[..., :3], ref).max())
    if not err <= tol:
        fails.append((what, f"colour error {err:.3g} > {tol}"))
    if err >= worst.get(what[2], (0.0, None))[0]:
        worst[what[2]] = (err, f"{c.name} / {what[1]}")
    for name, other, osteps in frames[1:]:
        if not (_bits(other) == _bits(img)).all():
            fails.append((what, f"policy '{name}' differs from '{frames[0][0]}' at {int((_bits(other) != _bits(img)).any(axis=2).sum())} pixels"))
        if not (osteps == steps).all():
            fails.append((what, f"policy '{name}': steps differ at {int((osteps != steps).sum())} pixels"))
    if not (_bits(prod) == _bits(img)).all():
        fails.append((what, "the production kernel differs from the COUNT kernel"))


def _report(title, fails, worst, runs, start):
    print(f"\n{title}: {runs} case x layout x family runs, {time.perf_counter() - start:.1f} s; largest colour error vs the references: "
          + ", ".join(f"{k} {e:.3g} ({n})" for k, (e, n) in worst.items()))
    for what, msg in fails[:40]:
        print("FAIL", what[0].name, what[1:], msg)
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"


def test_builtin_and_table_on_every_case(V, O, tf_lib):  # noqa: F811
    start = time.perf_counter()
    fails, worst, runs, sides = [], {}, 0, []
    for c in FC.cases():
        (ref, ref_steps), (tref, tref_steps) = references(O, tf_lib, c)
        for lay in _layouts(c):
            for family, setup, r, rs, tol in (("built-in", lambda ctx: None, ref, ref_steps, TOL),
                                              ("table", lambda ctx: ctx.set_transfer_function(FC.table(), FC.DOMAIN), tref, tref_steps, TOL_UNLIT)):
                what = (c, lay, family)
                ctx = _context(V, O, c, lay, setup)
                try:
                    sides.append(_check_path(V, O, ctx, c, what, fails))
                    _check_frames(V, ctx, c, what, r, rs, tol, fails, worst)
                finally:
                    ctx.close()
                runs += 1
    assert runs == 2 * sum(len(_layouts(c)) for c in FC.cases()) and any(sides) and not all(sides)
    _report("fastpath, built-in and table", fails, worst, runs, start)


@pytest.fixture(scope="module")
def family_libs(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("fastpath_gpu")
    return dict(lit=lit_helpers.build_restatement(d, O), mip=MH.build_restatement(d, O), shadow=SH.build_restatement(d, O), geom=GH.build_restatement(d, O))


def test_lit_max_iso_shadow_and_geometry_on_a_long_axis_and_a_far_camera(V, O, family_libs):
    start = time.perf_counter()
    fails, worst, runs = [], {}, 0
    for c in FC.family_cases():
        cam = c.blob(O)
        if c.u16:  # (the lit and MAX restatements have no R16_UNORM: the numpy references on the u16 scale)
            lit_ref, lit_steps = NU.render_table(None, cam, c.vol, c.W, c.H, table=FC.table(), domain=FC.DOMAIN, dt=c.dt, light=LIGHT)
            mip_ref, mip_steps, _ = NU.render_mip(None, cam, c.vol, c.W, c.H, dt=c.dt)
        else:
            lit_ref, lit_steps = lit_helpers.restate(family_libs["lit"], O, cam, c.vol, c.W, c.H, table=FC.table(), dt=c.dt, domain=FC.DOMAIN,
                                                     light=lit_helpers.light_vector(**LIGHT))
            mip_ref, mip_steps, _, _ = MH.restate(family_libs["mip"], O, cam, c.vol, c.W, c.H, dt=c.dt)
        iso_ref, iso_steps, _, iso_flags, _, _ = SH.restate(family_libs["shadow"], O, cam, c.vol, c.W, c.H, iso=ISO, colour=COLOUR, refine=REFINE, dt=c.dt, light=LIGHT)
        sh_ref, sh_steps, _, _, sh_iters, _ = SH.restate(family_libs["shadow"], O, cam, c.vol, c.W, c.H, iso=ISO, colour=COLOUR, refine=REFINE, dt=c.dt, light=LIGHT,
                                                         shadows=SHADOWS)
        geo_ref, geo_steps, _, _ = GH.restate(family_libs["geom"], O, cam, c.vol, c.W, c.H, iso=ISO, refine=REFINE, dt=c.dt)
        # the references alone: rays that cross at least half the long axis (max(dims) / dt_scale trips end to end), rays that march a quarter
        # of it before they hit, and shadow rays that march
        whole = max(c.dims) / c.dt
        assert int(mip_steps.max()) >= whole / 2 and int(iso_steps.max()) >= whole / 4 and (iso_flags & 2).any() and int(sh_iters.max()) >= 10, c

        def lit(ctx):
            ctx.set_transfer_function(FC.table(), FC.DOMAIN)
            ctx.set_lighting(**LIGHT)

        def iso(ctx):
            ctx.set_isosurface(ISO, COLOUR, REFINE)
            ctx.set_lighting(**LIGHT)

        def shadow(ctx):
            iso(ctx)
            ctx.set_shadows(*SHADOWS)

        for lay in _layouts(c):
            for family, setup, r, rs, tol in (("lit", lit, lit_ref, lit_steps, TOL_LIT), ("max", lambda ctx: ctx.set_projection("max"), mip_ref, mip_steps, TOL_MIP),
                                              ("iso", iso, iso_ref, iso_steps, TOL_LIT), ("iso+shadows", shadow, sh_ref, sh_steps, TOL_LIT)):
                what = (c, lay, family)
                ctx = _context(V, O, c, lay, setup)
                try:
                    _check_path(V, O, ctx, c, what, fails)
                    _check_frames(V, ctx, c, what, r[..., :3], rs, tol, fails, worst)
                    if family == "iso":  # the geometry pass: the restatement's records bit for bit, under every policy
                        for name, flags in _policies(V):
                            ctx.render_geometry(c.dt, None, flags)
                            pos_t, grad_x = ctx.read_geometry()
                            same = GH.same_bits(np.stack([pos_t, grad_x], axis=2), geo_ref)
                            if not same.all():
                                fails.append(((c, lay, "geometry"), f"policy '{name}': records differ from the restatement at {int((~same).any(axis=(1, 2)).sum())} pixels"))
                        runs += 1
                finally:
                    ctx.close()
                runs += 1
    assert runs == 5 * sum(len(_layouts(c)) for c in FC.family_cases())
    _report("fastpath, the other families", fails, worst, runs, start)


def test_batch_with_one_camera_beyond_the_precision_limit(V, O):
    import torch

    blobs, far, W, H = FC.batch_cameras(O)
    vol = FC.volume((32, 32, 32))
    for lay in ("PACKED", "PACKED_PAIRS"):
        ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
        try:
            V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + lay))
            pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0)
            singles, paths = [], []
            for b in blobs:
                ctx.set_camera_blob(b)
                paths.append(ctx.march_path_fast(1.0, 0))
                pipe.record(ctx)
                singles.append(_bits(ctx.read_backbuffer()).copy())
            # the near singles take the unclamped build; the camera that decides for the batch -- its farthest -- the clamped one
            assert paths == [i != far for i in range(len(blobs))], (lay, paths)
            assert all(s[..., :3].any() for s in singles), lay  # every frame shows the volume
            frames = torch.full((len(blobs), H, W, 4), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            V.render_batch(ctx, pipe, blobs, frames.data_ptr(), tile_size=8)
            ctx.sync()
            torch.cuda.synchronize()
            got = frames.cpu().numpy().view(np.uint32)
            for i, s in enumerate(singles):
                assert (got[i] == s).all(), (lay, i, int((got[i] != s).any(axis=2).sum()))
        finally:
            ctx.close()
