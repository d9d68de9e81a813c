"""The built-in transfer function of VK_MODE_NAIVE_TRILINEAR (no table) on the MI355X over the shared fuzz cases (tests/builtin_cases.py),
against the C oracle, which the CPU suite holds to an independent numpy reference (tests/test_builtin_fuzz_cpu.py).

For every case and every layout its format allows (u8: LINEAR, PACKED, PACKED_PAIRS, BRICKED, QUADS, STAGED; f16: all but PACKED_PAIRS):
- per-pixel step counts equal the oracle's, under every skip policy;
- colour within TOL of the oracle, and finite everywhere;
- every layout gives the LINEAR frame and step counts bit for bit (STAGED also with a 2 KiB window on a third of the cases, and with
  windows shared by a group of four waves on another third);
- on PACKED and PACKED_PAIRS, the default policy, RENDER_NO_SKIP, RENDER_FORCE_SKIP, RENDER_FORCE_SKIP | RENDER_PROBE_ALWAYS and
  RENDER_SAFE give bitwise-equal frames, and under FORCE_SKIP | PROBE_ALWAYS S_sampled is the oracle's count of steps in non-empty cells;
- the production kernel (no RENDER_COUNT) gives the COUNT kernel's frame bit for bit;
- RGBA16F output is the round-to-nearest-even of the RGBA32F frame (the cases marked `half`);
- the packed layouts report the empty fraction the case is built for;
- pixels outside a tile keep the clear colour;
- on the packed layouts of the edge cases, a table set and then reset with None leaves the frame, the step counts, S_sampled and the empty
  fraction of a fresh upload: cell_occ_kernel's built-in branch rebuilds what pack_cells_kernel built.
Every mismatch is collected and reported together with the case that shows it."""
import time

import numpy as np
import pytest

import builtin_cases
from gpu_helpers import TOL, V  # noqa: F401
from test_table_fuzz_cpu import rel_err, tile_mask
from test_transfer_gpu import _empty_fraction
from tf_helpers import band_pass_table

pytestmark = pytest.mark.gpu

U8_LAYOUTS = ("LINEAR", "PACKED", "PACKED_PAIRS", "BRICKED", "QUADS", "STAGED")
F16_LAYOUTS = ("LINEAR", "PACKED", "BRICKED", "QUADS", "STAGED")
PACKED = ("PACKED", "PACKED_PAIRS")


def _policies(V, lay):
    # the first is the one whose S_sampled is held to the oracle; the others must reproduce its frame bit for bit
    if lay not in PACKED:
        return (("default", 0),)
    return (("force+probe", V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS), ("default", 0), ("no skip", V.RENDER_NO_SKIP),
            ("force", V.RENDER_FORCE_SKIP), ("safe", V.RENDER_SAFE))


def _context(V, c, layout, out, params=()):
    ctx = V.Context(c.W, c.H, backbuffer=(c.W, c.H), out_format=out)
    try:
        for k, v in params:
            ctx.set_param(k, v)
        V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout))
    except BaseException:
        ctx.close()
        raise
    return ctx


def _render(V, ctx, cam, c, flags):
    """(frame, steps, (S_ref, S_sampled)); steps and counts only under RENDER_COUNT."""
    from vokselis_amd import _native as N

    N.check(ctx.handle, N.lib().vk_backbuffer_clear(ctx.handle))
    ctx.set_camera_blob(cam)
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=c.dt, flags=flags).record(ctx, c.tile)
    if flags & V.RENDER_COUNT:
        return ctx.read_backbuffer().copy(), ctx.read_steps().copy(), ctx.step_counts()
    return ctx.read_backbuffer().copy(), None, None


def _staged_params(i):
    return (("2 KiB window", (("stage_cap_bytes", 2048),)),) if i % 3 == 0 else ((("group windows", (("stage_group", 1),)),) if i % 3 == 1 else ())


def _bits(a):
    return a.view(np.uint32)


def test_builtin_fuzz_against_the_oracle(V, O):
    start = time.perf_counter()
    fails, worst = [], {}
    runs = renders = halves = empties = resets = 0
    for i, c in enumerate(builtin_cases.cases(O)):
        cam = O.camera_blob(*c.cam)
        ref, ref_steps, ref_sampled = O.render(cam, c.vol, c.W, c.H, dt_scale=c.dt)
        m = np.ones((c.H, c.W), bool) if c.tile is None else tile_mask(c)
        linear = None
        for lay in F16_LAYOUTS if c.f16 else U8_LAYOUTS:
            for label, params in (("", ()),) + (_staged_params(i) if lay == "STAGED" else ()):
                what = (c, lay + (f" ({label})" if label else ""))
                ctx = _context(V, c, lay, V.OUT_RGBA32F, params)
                try:
                    ef = _empty_fraction(ctx) if lay in PACKED else None
                    frames = [(name, *_render(V, ctx, cam, c, fl | V.RENDER_COUNT)) for name, fl in _policies(V, lay)]
                    prod, _, _ = _render(V, ctx, cam, c, 0)
                finally:
                    ctx.close()
                runs += 1
                renders += len(frames) + 1
                _, img, steps, counts = frames[0]
                if c.empty is not None and ef is not None:
                    empties += 1
                    if ef != c.empty:
                        fails.append((what, f"empty fraction {ef}, want {c.empty}"))
                for name, _, osteps, _ in frames:
                    if not (osteps[m] == ref_steps[m]).all():
                        fails.append((what, f"policy '{name}': steps differ from the oracle at {int((osteps[m] != ref_steps[m]).sum())} pixels"))
                if not np.isfinite(img).all():
                    fails.append((what, "non-finite output"))
                err = float(rel_err(img[m][..., :3], ref[m][..., :3]).max())
                if not err <= TOL:
                    fails.append((what, f"colour error {err:.3g} > {TOL}"))
                if err >= worst.get(lay, (0.0, None))[0]:
                    worst[lay] = (err, c.name)
                if c.tile is not None and not (img[~m] == [0.0, 0.0, 0.0, 1.0]).all():
                    fails.append((what, "pixels outside the tile were written"))
                for name, other, osteps, _ in frames[1:]:
                    if not (_bits(other) == _bits(img)).all():
                        fails.append((what, f"policy '{name}' differs from '{frames[0][0]}' at {int((_bits(other) != _bits(img)).any(axis=2).sum())} pixels"))
                if lay in PACKED and counts[1] != int(ref_sampled[m].sum()):
                    fails.append((what, f"S_sampled {counts[1]}, the oracle's {int(ref_sampled[m].sum())}"))
                if not (_bits(prod) == _bits(img)).all():
                    fails.append((what, "the production kernel differs from the COUNT kernel"))
                if lay == "LINEAR":
                    linear = (img, steps)
                elif not ((_bits(img) == _bits(linear[0])).all() and (steps == linear[1]).all()):
                    fails.append((what, f"differs from LINEAR at {int((_bits(img) != _bits(linear[0])).any(axis=2).sum())} pixels, "
                                        f"steps at {int((steps != linear[1]).sum())}"))
                if c.half and not label:
                    ctx = _context(V, c, lay, V.OUT_RGBA16F)
                    try:
                        h, _, _ = _render(V, ctx, cam, c, 0)
                    finally:
                        ctx.close()
                    halves += 1
                    renders += 1
                    if not (h.view(np.uint16) == prod.astype(np.float16).view(np.uint16)).all():
                        fails.append((what, "RGBA16F output is not the RNE of the RGBA32F frame"))
                if c.edge and lay in PACKED:  # a table set and reset: the skip maps rebuilt by cell_occ_kernel's built-in branch
                    ctx = _context(V, c, lay, V.OUT_RGBA32F)
                    try:
                        ctx.set_transfer_function(band_pass_table())
                        ctx.set_transfer_function(None)
                        got, gsteps, gcounts = _render(V, ctx, cam, c, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS | V.RENDER_COUNT)
                        gef = _empty_fraction(ctx)
                    finally:
                        ctx.close()
                    resets += 1
                    renders += 1
                    if not ((_bits(got) == _bits(img)).all() and (gsteps == steps).all()):
                        fails.append((what, "after a table reset: the frame or the steps differ from a fresh upload's"))
                    if gcounts[1] != counts[1] or gef != ef:
                        fails.append((what, f"after a table reset: S_sampled {gcounts[1]} / empty fraction {gef}, fresh upload {counts[1]} / {ef}"))
    elapsed = time.perf_counter() - start
    n = builtin_cases.N_CASES
    print(f"\nbuilt-in fuzz: {n} cases, {runs} case x layout runs, {renders} renders, {elapsed:.1f} s; largest colour error vs the oracle: "
          + ", ".join(f"{lay} {e:.3g} ({name})" for lay, (e, name) in worst.items()))
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    n_f16 = sum(c.f16 for c in builtin_cases.cases(O))
    n_staged = sum(len(_staged_params(i)) for i in range(n))
    assert runs == 6 * (n - n_f16) + 5 * n_f16 + n_staged and halves >= 10 and empties >= 6 and resets >= 20
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
