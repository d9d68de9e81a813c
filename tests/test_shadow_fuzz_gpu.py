"""The shadow kernels (raymarch_iso_shadow_kernel, raymarch_u16_iso_shadow_kernel) on the MI355X over the shared fuzz cases
(tests/shadow_cases.py), against the C restatement (tests/shadow_restatement.c), which the CPU suite holds to an independent numpy
reference (tests/test_shadow_fuzz_cpu.py).

For every case and every layout with isosurface kernels (u8: LINEAR, PACKED, PACKED_PAIRS; f16 and u16: LINEAR, PACKED), rendered through
the Python API with set_isosurface, set_lighting, set_shadows and set_clip_box:
- per-pixel step counts equal the restatement's: they are the primary ray's, shadows must not move them;
- under FORCE_SKIP | PROBE_ALWAYS the packed layouts' (S_ref, S_sampled) is what tests/test_iso_fuzz_gpu.py expects without shadows: the
  restatement's step sum and the number of primary iterations whose cell is not empty under the isosurface's predicate;
- colour within TOL_LIT = 1e-4 per channel relative to max(1, |ref|) at every pixel of the tile, and finite; alpha is 1; pixels outside
  the tile stay untouched;
- the default policy, RENDER_NO_SKIP, RENDER_FORCE_SKIP | RENDER_PROBE_ALWAYS and RENDER_SAFE give bitwise-equal frames: this is what
  holds the shadow march's skipping to exactness;
- the production kernel (no RENDER_COUNT) gives the COUNT kernel's frame bit for bit;
- RGBA16F output is the round-to-nearest-even of the RGBA32F frame (the cases marked `half`);
- the mask cases (ambient 0, specular 0, diffuse 1, strength 1, colour 1): the set of hit pixels that are exactly (0, 0, 0) equals the
  restatement's shadow mask, pixels whose restated |N.L| is 0 excluded (at most 1 % of a case's hits: tests/test_shadow_fuzz_cpu.py).
  No tolerance: every operation that decides the mask is specified in f32.
Every mismatch is collected and reported together with the case that shows it."""
import time

import numpy as np
import pytest

import np_shadow_reference as NS
import shadow_cases
import shadow_helpers as SH
from gpu_helpers import V  # noqa: F401
from test_table_fuzz_cpu import rel_err, tile_mask
from test_table_fuzz_gpu import TOL_LIT, _policies

pytestmark = pytest.mark.gpu

LAYOUTS = {"u8": ("LINEAR", "PACKED", "PACKED_PAIRS"), "f16": ("LINEAR", "PACKED"), "u16": ("LINEAR", "PACKED")}


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("shadow_fuzz_gpu"), O)


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
        ctx.set_lighting(**c.light)
        ctx.set_shadows(*c.shadows)
        if c.box is not None:
            ctx.set_clip_box(*c.box)
        kw = dict(fmt=V.FMT_R16_UNORM) if c.kind == "u16" else {}
        V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout), **kw)
    except BaseException:
        ctx.close()
        raise
    return ctx


def test_shadow_fuzz_against_the_restatement(V, O, lib):  # noqa: F811
    start = time.perf_counter()
    fails, worst = [], (0.0, None)
    runs = halves = sampled_checks = masks = mask_pixels = 0
    cases = shadow_cases.cases(O)
    for c in cases:
        cam = O.camera_blob(*c.cam)
        ref4, ref_steps, _, fl, _, nl = SH.restate_case(lib, O, c)
        ref = ref4[..., :3]
        _, np_steps, live, _, _, _, _ = NS.render(cam, c.vol, c.W, c.H, iso=c.iso, colour=c.colour, refine=0, dt=c.dt, box=c.box)  # (no light: no shadows)
        m = np.ones((c.H, c.W), bool) if c.tile is None else tile_mask(c)
        assert np.isfinite(ref).all() and (np_steps == ref_steps).all()
        hit, dark = (fl & SH.HIT) != 0, (fl & SH.SHADOWED) != 0
        for lay in LAYOUTS[c.kind]:
            what = (c, lay)
            ctx = _context(V, c, lay, V.OUT_RGBA32F)
            try:
                frames = [(name, *_render(V, ctx, cam, c, fl_ | V.RENDER_COUNT)) for name, fl_ in _policies(V)]
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
            if err > TOL_LIT or np.isnan(err):
                fails.append((what, f"colour error {err:.3g} > {TOL_LIT}"))
            if err >= worst[0]:
                worst = (err, f"{c.name} / {lay}")
            if not (img[m][..., 3] == 1.0).all():
                fails.append((what, "alpha is not 1"))
            if c.tile is not None and not (img[~m] == [0.0, 0.0, 0.0, 1.0]).all():
                fails.append((what, "pixels outside the tile were written"))
            if lay != "LINEAR":  # force + probe always: a primary trip samples exactly when its cell is not empty; shadow trips count in neither
                sampled_checks += 1
                want = (int(ref_steps[m].sum()), int(live[m].sum()))
                if counts != want:
                    fails.append((what, f"(S_ref, S_sampled) = {counts}, want {want}"))
            for name, other, osteps, _ in frames[1:]:
                if not (other.view(np.uint32) == img.view(np.uint32)).all():
                    fails.append((what, f"policy '{name}' differs from '{frames[0][0]}' at {int((other.view(np.uint32) != img.view(np.uint32)).any(axis=2).sum())} pixels"))
                if not (osteps[m] == steps[m]).all():
                    fails.append((what, f"policy '{name}': steps differ"))
            if not (prod.view(np.uint32) == frames[1][1].view(np.uint32)).all():
                fails.append((what, "the production kernel differs from the COUNT kernel"))
            if c.mask:
                masks += 1
                sel = hit & m & ~(nl == 0)
                mask_pixels += int(sel.sum())
                black = (img[..., :3] == 0).all(axis=2)
                if not (black[sel] == dark[sel]).all():
                    fails.append((what, f"shadow mask differs from the restatement's at {int((black[sel] != dark[sel]).sum())} of {int(sel.sum())} hit pixels"))
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
    print(f"\nshadow fuzz: {len(cases)} cases, {runs} case x layout runs ({5 * runs + halves} renders), {elapsed:.1f} s; largest colour error vs "
          f"restatement {worst[0]:.3g} ({worst[1]}); {masks} mask runs over {mask_pixels} hit pixels")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    n_u8 = sum(c.kind == "u8" for c in cases)
    assert runs == 3 * n_u8 + 2 * (len(cases) - n_u8) and halves >= 7 and masks >= 24 and mask_pixels > 5000 and sampled_checks >= len(cases)
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
