"""The table kernels (raymarch_tf_kernel) and the lit kernels (raymarch_lit_kernel) on the MI355X over the shared fuzz cases
(tests/table_cases.py), against the C restatements (tests/tf_restatement.c unlit, tests/lit_restatement.c lit), which the CPU suite holds
to an independent numpy reference (tests/test_table_fuzz_cpu.py).

For every case and every layout with table kernels (u8: LINEAR, PACKED, PACKED_PAIRS; f16: LINEAR, PACKED), rendered through the Python
API with set_transfer_function and set_lighting:
- per-pixel step counts equal the restatement's, under every skip policy;
- colour within 1e-5 per channel unlit and 1e-4 lit, relative to max(1, |ref|), and finite wherever the restatement's is;
- the default policy, RENDER_NO_SKIP, RENDER_FORCE_SKIP | RENDER_PROBE_ALWAYS and RENDER_SAFE give bitwise-equal frames;
- the production kernel (no RENDER_COUNT) gives the COUNT kernel's frame bit for bit;
- RGBA16F output is the round-to-nearest-even of the RGBA32F frame, bit for bit (the cases marked `half`);
- the packed layouts report the empty fraction the case is built for (1.0: every cell empty; 0.0: none).
Every mismatch is collected and reported together with the case that shows it."""
import time

import numpy as np
import pytest

import table_cases
from gpu_helpers import V  # noqa: F401
from test_table_fuzz_cpu import libs, rel_err, restate, tile_mask  # noqa: F401
from test_transfer_gpu import _empty_fraction

pytestmark = pytest.mark.gpu

TOL_UNLIT, TOL_LIT = 1e-5, 1e-4
U8_LAYOUTS, F16_LAYOUTS = ("LINEAR", "PACKED", "PACKED_PAIRS"), ("LINEAR", "PACKED")


def _policies(V):
    # the first is the one held to the restatement; the others must reproduce it bit for bit
    return (("force+probe", V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS), ("default", 0), ("no skip", V.RENDER_NO_SKIP), ("safe", V.RENDER_SAFE))


def _render(V, ctx, cam, c, flags):
    from vokselis_amd import _native as N

    N.check(ctx.handle, N.lib().vk_backbuffer_clear(ctx.handle))
    ctx.set_camera_blob(cam)
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=c.dt, flags=flags).record(ctx, c.tile)
    return ctx.read_backbuffer().copy(), (ctx.read_steps().copy() if flags & V.RENDER_COUNT else None)


def _context(V, c, layout, out):
    ctx = V.Context(c.W, c.H, backbuffer=(c.W, c.H), out_format=out)
    try:
        ctx.set_transfer_function(c.table, c.domain)
        if c.light is not None:
            ctx.set_lighting(**c.light)
        V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout))
    except BaseException:
        ctx.close()
        raise
    return ctx


def test_table_fuzz_against_the_restatement(V, O, libs):  # noqa: F811
    start = time.perf_counter()
    fails, worst = [], {"unlit": (0.0, None), "lit": (0.0, None)}
    runs = halves = empties = 0
    for c in table_cases.cases(O):
        cam = O.camera_blob(*c.cam)
        ref, ref_steps = restate(libs, O, c)
        m = np.ones((c.H, c.W), bool) if c.tile is None else tile_mask(c)
        kind, tol = ("unlit", TOL_UNLIT) if c.light is None else ("lit", TOL_LIT)
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
                prod, _ = _render(V, ctx, cam, c, 0)
            finally:
                ctx.close()
            runs += 1
            _, img, steps = frames[0]
            if not (steps[m] == ref_steps[m]).all():
                fails.append((what, f"steps differ from the restatement at {int((steps[m] != ref_steps[m]).sum())} pixels"))
            fin = np.isfinite(ref[m])
            if not np.isfinite(img[m][..., :3][fin]).all():
                fails.append((what, "non-finite output where the restatement is finite"))
            err = float(rel_err(img[m][..., :3][fin], ref[m][fin]).max()) if fin.any() else 0.0
            if err > tol or np.isnan(err):
                fails.append((what, f"colour error {err:.3g} > {tol}"))
            if err >= worst[kind][0]:
                worst[kind] = (err, f"{c.name} / {lay}")
            if c.tile is not None and not (img[~m] == [0.0, 0.0, 0.0, 1.0]).all():
                fails.append((what, "pixels outside the tile were written"))
            for name, other, osteps in frames[1:]:
                if not (other.view(np.uint32) == img.view(np.uint32)).all():
                    fails.append((what, f"policy '{name}' differs from '{frames[0][0]}' at {int((other.view(np.uint32) != img.view(np.uint32)).any(axis=2).sum())} pixels"))
                if not (osteps[m] == steps[m]).all():
                    fails.append((what, f"policy '{name}': steps differ"))
            if not (prod.view(np.uint32) == frames[1][1].view(np.uint32)).all():
                fails.append((what, "the production kernel differs from the COUNT kernel"))
            if c.half:
                ctx = _context(V, c, lay, V.OUT_RGBA16F)
                try:
                    h, _ = _render(V, ctx, cam, c, 0)
                finally:
                    ctx.close()
                halves += 1
                if not (h.view(np.uint16) == prod.astype(np.float16).view(np.uint16)).all():
                    fails.append((what, "RGBA16F output is not the RNE of the RGBA32F frame"))
    elapsed = time.perf_counter() - start
    print(f"\ntable fuzz: {len(table_cases.cases(O))} cases, {runs} case x layout runs ({5 * runs + halves} renders), {elapsed:.1f} s; largest colour "
          f"error vs restatement: unlit {worst['unlit'][0]:.3g} ({worst['unlit'][1]}), lit {worst['lit'][0]:.3g} ({worst['lit'][1]})")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    n_f16 = sum(c.f16 for c in table_cases.cases(O))
    assert runs == 3 * (table_cases.N_CASES - n_f16) + 2 * n_f16 and halves >= 2 and empties >= 4
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
