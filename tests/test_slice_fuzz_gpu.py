"""The slice kernels (slice_kernel of vk_launch_slice.hip) on the MI355X over the shared cases (tests/slice_cases.py), against the C
restatement (tests/slice_restatement.c), which the CPU suite holds to an independent numpy reference (tests/test_slice_fuzz_cpu.py).

For every case and every layout of its format (u8: LINEAR, PACKED, PACKED_PAIRS; f16 and u16: LINEAR, PACKED), rendered through the Python
API into an RGBA32F backbuffer with values=True, under the case's table and clip box:
- the value surface equals the restatement's BIT FOR BIT at every pixel of the tile (a NaN x -- a cell with a non-finite tap -- is held to
  "is a NaN": which NaN an invalid operation yields is the one thing left open, tests/geom_helpers.py: same_bits);
- colour is within the unlit table kernels' bar, TOL_UNLIT, relative to max(1, |ref|), alpha exactly 1;
- pixels of the backbuffer and of the value surface outside the tile are bitwise what they held before the pass;
- on the cases marked `half`, the RGBA16F frame is the round-to-nearest-even of the f32 frame;
- all layouts of a format give bitwise-equal frames and value surfaces.
The run count and a floor on the inside pixels are asserted, so an empty loop cannot pass.  Every mismatch is collected and reported
together with the case that shows it."""
import time

import numpy as np
import pytest

import slice_cases
import slice_helpers as SH
from gpu_helpers import V  # noqa: F401
from test_table_fuzz_gpu import TOL_UNLIT

pytestmark = pytest.mark.gpu

LAYOUTS = {"u8": ("LINEAR", "PACKED", "PACKED_PAIRS"), "f16": ("LINEAR", "PACKED"), "u16": ("LINEAR", "PACKED")}


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("slice_fuzz_gpu"), O)


def context(V, c, layout, out_format):  # noqa: F811
    ctx = V.Context(c.W, c.H, backbuffer=(c.W, c.H), out_format=out_format)
    try:
        if c.table is not None:
            ctx.set_transfer_function(c.table, c.domain)
        if c.box is not None:
            ctx.set_clip_box(*c.box)
        kw = dict(fmt=V.FMT_R16_UNORM) if c.kind == "u16" else {}
        V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout), **kw)
    except BaseException:
        ctx.close()
        raise
    return ctx


def test_slice_fuzz_against_the_restatement(V, O, lib):  # noqa: F811
    start = time.perf_counter()
    fails = []
    runs = inside = halves = expected_inside = 0
    worst = (0.0, None)
    cases = slice_cases.cases(O)
    for c in cases:
        ref_rgba, ref_val, _, fl = SH.restate_case(lib, c, tile=True)
        m = SH.tile_mask(c)
        s = SH.vk_slice(V, c)
        first = None
        for lay in LAYOUTS[c.kind]:
            what = (c, lay)
            ctx = context(V, c, lay, V.OUT_RGBA32F)
            try:
                before = ctx.read_backbuffer().copy()  # the cleared backbuffer
                ctx.render_slice(s, c.tile, values=True)
                img, val = ctx.read_backbuffer(), ctx.read_slice_values()
            finally:
                ctx.close()
            runs += 1
            expected_inside += int(((fl & SH.INSIDE) != 0).sum())
            inside += int((val[..., 1] != 0).sum())
            same = SH.same_bits(val, ref_val)
            if not same[m].all():
                bad = ~same[m]
                fails.append((what, f"value records differ from the restatement at {int(bad.any(axis=1).sum())} pixels of the tile (x words {int(bad[:, 0].sum())}, weight words {int(bad[:, 1].sum())})"))
            if not ((val[..., 1] != 0) == ((fl & SH.INSIDE) != 0)).all():
                fails.append((what, "the weights are not the restatement's inside mask"))
            if not (val[~m].view(np.uint32) == 0).all():
                fails.append((what, "value records outside the tile were written"))
            if not (img[~m].view(np.uint32) == before[~m].view(np.uint32)).all():
                fails.append((what, "backbuffer pixels outside the tile were written"))
            if not (np.isfinite(img).all() and (img[m][:, 3] == 1.0).all()):
                fails.append((what, "a colour is not finite or alpha is not 1"))
            err = float(SH.rel_err(img[m][:, :3], ref_rgba[m][:, :3]).max(initial=0.0))
            if not err <= TOL_UNLIT:
                fails.append((what, f"colour error {err:.3g} above {TOL_UNLIT}"))
            if err >= worst[0]:
                worst = (err, f"{c.name} {lay}")
            if first is None:
                first = (lay, img, val)
            elif not ((img.view(np.uint32) == first[1].view(np.uint32)).all() and SH.same_bits(val, first[2]).all()):
                fails.append((what, f"differs bitwise from layout {first[0]}"))
            if c.half:
                ctx = context(V, c, lay, V.OUT_RGBA16F)
                try:
                    ctx.render_slice(s, c.tile, values=True)
                    img16, val16 = ctx.read_backbuffer(), ctx.read_slice_values()
                finally:
                    ctx.close()
                halves += 1
                with np.errstate(over="ignore"):
                    want16 = img.astype(np.float16)  # numpy rounds to nearest even
                if not (img16.view(np.uint16) == want16.view(np.uint16)).all():
                    fails.append((what, f"the RGBA16F frame is not the rounded f32 frame at {int((img16.view(np.uint16) != want16.view(np.uint16)).any(axis=2).sum())} pixels"))
                if not SH.same_bits(val16, val).all():
                    fails.append((what, "the value surface depends on the output format"))
    elapsed = time.perf_counter() - start
    print(f"\nslice fuzz: {len(cases)} cases, {runs} case x layout runs, {halves} half-float runs, {inside} inside pixels held bit for bit, "
          f"largest colour error {worst[0]:.3g} ({worst[1]}), {elapsed:.1f} s")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    n_u8 = sum(c.kind == "u8" for c in cases)
    assert runs == 3 * n_u8 + 2 * (len(cases) - n_u8) and halves >= 6 and inside == expected_inside and inside > 20000
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
