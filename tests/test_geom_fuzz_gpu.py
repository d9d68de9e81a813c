"""The geometry kernels (raymarch_geom_kernel, raymarch_u16_geom_kernel and their _clip_ twins) on the MI355X over the shared cases
(tests/geom_cases.py), against the C restatement (tests/geom_restatement.c), which the CPU suite holds to an independent numpy reference
(tests/test_geom_fuzz_cpu.py).

For every case and every layout with isosurface kernels (u8: LINEAR, PACKED, PACKED_PAIRS; f16 and u16: LINEAR, PACKED), rendered through
the Python API with set_isosurface, the case's lighting (set or not: the pass ignores it) and set_clip_box:
- both float4 of every pixel of the tile equal the restatement's BIT FOR BIT, the gradient included: the build uses -ffp-contract=off and
  the gradient is specified operation by operation.  (A NaN component -- a cell with a non-finite tap -- is held to "is a NaN": which
  NaN an invalid operation yields is the one thing left open, tests/geom_helpers.py: same_bits.)
- the default policy, RENDER_NO_SKIP, RENDER_FORCE_SKIP | RENDER_PROBE_ALWAYS and RENDER_SAFE give bitwise-equal surfaces;
- pixels outside the tile keep the miss record;
- the backbuffer is bitwise what it held before the pass.
Every mismatch is collected and reported together with the case that shows it."""
import time

import numpy as np
import pytest

import geom_cases
import geom_helpers as GH
from gpu_helpers import V  # noqa: F401
from test_table_fuzz_gpu import _policies

pytestmark = pytest.mark.gpu

LAYOUTS = {"u8": ("LINEAR", "PACKED", "PACKED_PAIRS"), "f16": ("LINEAR", "PACKED"), "u16": ("LINEAR", "PACKED")}


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return GH.build_restatement(tmp_path_factory.mktemp("geom_fuzz_gpu"), O)


def _context(V, c, layout):
    ctx = V.Context(c.W, c.H, backbuffer=(c.W, c.H), out_format=V.OUT_RGBA32F)
    try:
        ctx.set_isosurface(c.iso, (0.9, 0.6, 0.3), c.refine)
        if c.light is not None:
            ctx.set_lighting(**c.light)
        if c.box is not None:
            ctx.set_clip_box(*c.box)
        kw = dict(fmt=V.FMT_R16_UNORM) if c.kind == "u16" else {}
        V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout), **kw)
    except BaseException:
        ctx.close()
        raise
    return ctx


def test_geometry_fuzz_against_the_restatement(V, O, lib):  # noqa: F811
    start = time.perf_counter()
    fails = []
    runs = hits = 0
    cases = geom_cases.cases(O)
    for c in cases:
        cam = O.camera_blob(*c.cam)
        ref, _, _, fl = GH.restate_case(lib, O, c, tile=True)
        m = GH.tile_mask(c)
        for lay in LAYOUTS[c.kind]:
            what = (c, lay)
            ctx = _context(V, c, lay)
            try:
                ctx.set_camera_blob(cam)
                V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=c.dt).record(ctx)  # a colour frame for the pass to leave alone
                before = ctx.read_backbuffer().copy()
                surfaces = []
                for name, flags in _policies(V):
                    ctx.render_geometry(c.dt, c.tile, flags)
                    pos_t, grad_x = ctx.read_geometry()
                    surfaces.append((name, np.stack([pos_t, grad_x], axis=2)))
                after = ctx.read_backbuffer()
            finally:
                ctx.close()
            runs += 1
            _, got = surfaces[0]
            hits += int(np.isfinite(got[:, :, 0, 3]).sum())
            same = GH.same_bits(got, ref)
            if not same[m].all():
                bad = ~same[m]
                fails.append((what, f"records differ from the restatement at {int(bad.any(axis=(1, 2)).sum())} pixels of the tile "
                                    f"(position/t words {int(bad[:, 0, :].sum())}, gradient words {int(bad[:, 1, :3].sum())}, value words {int(bad[:, 1, 3].sum())})"))
            if not GH.same_bits(got[~m], GH.MISS).all():
                fails.append((what, "pixels outside the tile were written"))
            if not (np.isfinite(got[:, :, 0, 3]) == ((fl & GH.HIT) != 0)).all():
                fails.append((what, "isfinite(t) is not the restatement's hit mask"))
            for name, other in surfaces[1:]:
                if not (other.view(np.uint32) == got.view(np.uint32)).all():
                    fails.append((what, f"policy '{name}' differs from '{surfaces[0][0]}' at {int((other.view(np.uint32) != got.view(np.uint32)).any(axis=(2, 3)).sum())} pixels"))
            if not (after.view(np.uint32) == before.view(np.uint32)).all():
                fails.append((what, "the pass wrote the backbuffer"))
    elapsed = time.perf_counter() - start
    print(f"\ngeometry fuzz: {len(cases)} cases, {runs} case x layout runs ({4 * runs} passes), {hits} hit pixels held bit for bit, {elapsed:.1f} s")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    n_u8 = sum(c.kind == "u8" for c in cases)
    assert runs == 3 * n_u8 + 2 * (len(cases) - n_u8) and hits > 50000
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
