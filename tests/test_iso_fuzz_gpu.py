"""The isosurface kernels (raymarch_iso_kernel) on the MI355X over the shared fuzz cases (tests/iso_cases.py), against the C restatement
(tests/iso_restatement.c), which the CPU suite holds to an independent numpy reference (tests/test_iso_fuzz_cpu.py).

For every case and every layout with isosurface kernels (u8: LINEAR, PACKED, PACKED_PAIRS; f16: LINEAR, PACKED), rendered through the
Python API with set_isosurface and set_lighting:
- per-pixel step counts equal the restatement's, under every skip policy;
- colour within 1e-5 unlit and 1e-4 lit per channel relative to max(1, |ref|) (the bars of the table kernels: the shade is the same
  lit_shade, once per ray) at every pixel of the tile, and finite; alpha is 1;
- the default policy, RENDER_NO_SKIP, RENDER_FORCE_SKIP | RENDER_PROBE_ALWAYS and RENDER_SAFE give bitwise-equal frames;
- the production kernel (no RENDER_COUNT) gives the COUNT kernel's frame bit for bit;
- RGBA16F output is the round-to-nearest-even of the RGBA32F frame (the cases marked `half`); pixels outside the tile stay untouched;
- the packed layouts report the empty fraction the case is built for, and under FORCE_SKIP | PROBE_ALWAYS their (S_ref, S_sampled) is the
  restatement's step sum and the number of iterations whose cell is not empty under the isosurface's predicate, as
  tests/np_iso_reference.py counts them from each sample's eight taps.
Every mismatch is collected and reported together with the case that shows it."""
import time

import numpy as np
import pytest

import iso_cases
import iso_helpers as IH
import np_iso_reference as NI
from gpu_helpers import V  # noqa: F401
from test_table_fuzz_cpu import rel_err, tile_mask
from test_table_fuzz_gpu import TOL_LIT, TOL_UNLIT, _policies
from test_transfer_gpu import _empty_fraction

pytestmark = pytest.mark.gpu

U8_LAYOUTS, F16_LAYOUTS = ("LINEAR", "PACKED", "PACKED_PAIRS"), ("LINEAR", "PACKED")


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return IH.build_restatement(tmp_path_factory.mktemp("iso_fuzz_gpu"), O)


def _render(V, ctx, cam, c, flags):
    from vokselis_amd import _native as N

    N.check(ctx.handle, N.lib().vk_backbuffer_clear(ctx.handle))
    ctx.set_camera_blob(cam)
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=c.dt, flags=flags).record(ctx, c.tile)
    counted = bool(flags & V.RENDER_COUNT)
    return ctx.read_backbuffer().copy(), (ctx.read_steps().copy() if counted else None), (ctx.step_counts() if counted else None)


def _context(V, c, layout, out):
    ctx = V.Context(c.W, c.H, backbuffer=(c.W, c.H), out_format=out)
    try:
        ctx.set_isosurface(c.iso, c.colour, c.refine)
        if c.light is not None:
            ctx.set_lighting(**c.light)
        V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout))
    except BaseException:
        ctx.close()
        raise
    return ctx


def test_iso_fuzz_against_the_restatement(V, O, lib):  # noqa: F811
    start = time.perf_counter()
    fails, worst = [], {False: (0.0, None), True: (0.0, None)}
    runs = halves = empties = sampled_checks = 0
    for c in iso_cases.cases(O):
        cam = O.camera_blob(*c.cam)
        ref4, ref_steps, _, _ = IH.restate_case(lib, O, c)
        ref = ref4[..., :3]
        _, np_steps, live, _, _ = NI.render(cam, c.vol, c.W, c.H, iso=c.iso, colour=c.colour, refine=0, dt=c.dt)
        m = np.ones((c.H, c.W), bool) if c.tile is None else tile_mask(c)
        assert np.isfinite(ref).all() and (np_steps == ref_steps).all()
        lit = c.light is not None
        tol = TOL_LIT if lit else TOL_UNLIT
        for lay in F16_LAYOUTS if c.f16 else U8_LAYOUTS:
            what = (c, lay)
            ctx = _context(V, c, lay, V.OUT_RGBA32F)
            try:
                if c.empty is not None and lay != "LINEAR":
                    ef = _empty_fraction(ctx)
                    empties += 1
                    if ef != c.empty:
                        fails.append((what, f"empty fraction {ef}, want {c.empty}"))
                frames = [(name, *_render(V, ctx, cam, c, fl | V.RENDER_COUNT)) for name, fl in _policies(V)]
                prod, _, _ = _render(V, ctx, cam, c, 0)
            finally:
                ctx.close()
            runs += 1
            _, img, steps, counts = frames[0]
            if not (steps[m] == ref_steps[m]).all():
                fails.append((what, f"steps differ from the restatement at {int((steps[m] != ref_steps[m]).sum())} pixels"))
            if not np.isfinite(img[m][..., :3]).all():
                fails.append((what, "non-finite output"))
            err = float(rel_err(img[m][..., :3], ref[m]).max())
            if err > tol or np.isnan(err):
                fails.append((what, f"colour error {err:.3g} > {tol}"))
            if err >= worst[lit][0]:
                worst[lit] = (err, f"{c.name} / {lay}")
            if not (img[m][..., 3] == 1.0).all():
                fails.append((what, "alpha is not 1"))
            if c.tile is not None and not (img[~m] == [0.0, 0.0, 0.0, 1.0]).all():
                fails.append((what, "pixels outside the tile were written"))
            if lay != "LINEAR":  # force + probe always: a trip samples exactly when its cell is not empty
                sampled_checks += 1
                want_ref, want_samp = int(ref_steps[m].sum()), int(live[m].sum())
                if counts != (want_ref, want_samp):
                    fails.append((what, f"(S_ref, S_sampled) = {counts}, want {(want_ref, want_samp)}"))
                if c.empty is not None and want_samp != (0 if c.empty == 1.0 else want_ref):
                    fails.append((what, f"the reference counts {want_samp} sampled iterations of {want_ref}: the case is not what it is built for"))
            for name, other, osteps, _ in frames[1:]:
                if not (other.view(np.uint32) == img.view(np.uint32)).all():
                    fails.append((what, f"policy '{name}' differs from '{frames[0][0]}' at {int((other.view(np.uint32) != img.view(np.uint32)).any(axis=2).sum())} pixels"))
                if not (osteps[m] == steps[m]).all():
                    fails.append((what, f"policy '{name}': steps differ"))
            if not (prod.view(np.uint32) == frames[1][1].view(np.uint32)).all():
                fails.append((what, "the production kernel differs from the COUNT kernel"))
            if c.half:
                ctx = _context(V, c, lay, V.OUT_RGBA16F)
                try:
                    h, _, _ = _render(V, ctx, cam, c, 0)
                finally:
                    ctx.close()
                halves += 1
                if not (h.view(np.uint16) == prod.astype(np.float16).view(np.uint16)).all():
                    fails.append((what, "RGBA16F output is not the RNE of the RGBA32F frame"))
    elapsed = time.perf_counter() - start
    print(f"\nisosurface fuzz: {len(iso_cases.cases(O))} cases, {runs} case x layout runs ({5 * runs + halves} renders), {elapsed:.1f} s; largest "
          f"colour error vs restatement unlit {worst[False][0]:.3g} ({worst[False][1]}), lit {worst[True][0]:.3g} ({worst[True][1]})")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    n_f16 = sum(c.f16 for c in iso_cases.cases(O))
    assert runs == 3 * (iso_cases.N_CASES - n_f16) + 2 * n_f16 and halves >= 4 and empties >= 6 and sampled_checks >= 2 * iso_cases.N_CASES - n_f16
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
