"""The two references of light-direction shadows under a first-hit isosurface held together over the shared fuzz cases
(tests/shadow_cases.py): the C restatement (tests/shadow_restatement.c: f32, the specification's operation order) and the numpy reference
(tests/np_shadow_reference.py: hit tests, positions and the loop variable exact in f32, the shade and sRGB in float64).

Step counts, the hit mask, the refined a, the shadow mask and the shadow iterations must be equal at every pixel.  Colour must agree within
the isosurface tests' lit bar, TOL_LIT = 1e-4 relative to max(1, |ref|), on EVERY pixel.  The conditions on the case list -- one pixel at
least of every kind of shadow ray -- are asserted on the restatement, so the list cannot quietly degenerate; the counts are printed."""
import numpy as np
import pytest

import np_shadow_reference as NS
import shadow_cases
import shadow_helpers as SH
from test_table_fuzz_cpu import TOL_LIT, rel_err, tile_mask


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("shadow_fuzz_cpu"), O)


@pytest.fixture(scope="module")
def restated(O, lib):
    return [SH.restate_case(lib, O, c) for c in shadow_cases.cases(O)]


@pytest.fixture(scope="module")
def referenced(O):
    return [NS.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, iso=c.iso, colour=c.colour, refine=c.refine, dt=c.dt, light=c.light, shadow=c.shadows,
                      box=c.box) for c in shadow_cases.cases(O)]


def test_case_list_covers_the_edges(O):
    cases = shadow_cases.cases(O)
    assert len(cases) == shadow_cases.N_CASES
    assert {c.dt for c in cases} == set(shadow_cases.DTS)
    assert {c.kind for c in cases} == {"u8", "f16", "u16"}
    for kind in ("u8", "f16", "u16"):
        assert any(c.kind == kind and c.half for c in cases) and any(c.kind == kind and c.box is not None for c in cases), kind
    for dims in shadow_cases.FIXED_DIMS:
        assert any(c.dims == dims for c in cases), dims
    assert max(max(c.dims) for c in cases) <= 65 and all(24 <= min(c.W, c.H) and max(c.W, c.H) <= 80 for c in cases)
    assert any(c.tile is not None and min(c.tile[:2]) < 0 for c in cases)
    assert any(c.tile is not None and min(c.tile[:2]) > 0 and c.tile[0] + c.tile[2] < c.W and c.tile[1] + c.tile[3] < c.H for c in cases)
    assert all(not isinstance(c.light["direction"], str) for c in cases)  # never a headlight: every case casts shadow rays
    assert {c.shadows[0] for c in cases} >= {0.0, 1.0} and {c.shadows[1] for c in cases} >= {0.0, 1024.0}
    assert any(c.light["direction"] == (1.0, 0.0, 0.0) for c in cases) and any(c.light["direction"] == (-1.0, 0.0, 0.0) for c in cases)
    assert any("random" in c.tags for c in cases)
    for c in cases:
        if c.mask:
            assert (c.light["ambient"], c.light["diffuse"], c.light["specular"], c.shadows[0], c.colour) == (0.0, 1.0, 0.0, 1.0, (1.0, 1.0, 1.0)), c
    assert sum(c.mask for c in cases) >= 8 and {c.kind for c in cases if c.mask} == {"u8", "f16", "u16"}


def test_case_list_conditions_hold_on_the_restatement(O, lib, restated):
    cases = shadow_cases.cases(O)
    n = dict(other=0, self_=0, lit_long=0, zero=0, miss=0, first_dark=0, first_lit=0, nan=0, pinf=0, hit=0, cast=0, dark=0)
    for c, (img, steps, a, fl, iters, nl) in zip(cases, restated):
        hit, cast, dark = (fl & SH.HIT) != 0, (fl & SH.CAST) != 0, (fl & SH.SHADOWED) != 0
        first, miss, zero = (fl & SH.FIRST) != 0, (fl & SH.MISS) != 0, (fl & SH.ZERO) != 0
        assert (cast == hit).all() and (dark <= cast).all() and (iters[~cast] == 0).all(), c
        assert (iters[dark] >= 1).all() and (iters[miss | zero] == 0).all() and not (dark & (miss | zero)).any(), c
        n["hit"] += int(hit.sum()); n["cast"] += int(cast.sum()); n["dark"] += int(dark.sum())
        n["other"] += int((dark & (nl > 0) & (iters >= 2)).sum())   # facing the light, yet a later shadow sample hits
        n["self_"] += int((dark & (nl < 0)).sum())                   # facing away
        n["lit_long"] += int((cast & ~dark & (iters >= 8)).sum())
        n["zero"] += int(zero.sum()); n["miss"] += int(miss.sum())
        n["first_dark"] += int((first & dark).sum()); n["first_lit"] += int((first & cast & ~dark).sum())
        n["nan"] += int(((fl & SH.NAN_SEEN) != 0).sum()); n["pinf"] += int(((fl & SH.PINF_HIT) != 0).sum())
        if c.name == "bias 0":
            assert hit.sum() > 100 and (dark == hit).all() and (iters[hit] == 1).all(), c
        if c.name == "bias 1024":
            assert hit.sum() > 100 and (zero | miss)[hit].all() and not dark.any(), c
        if c.name == "iso above all data":
            assert not hit.any() and not cast.any() and steps.max() > 1, c
        if c.shadows[0] == 0.0:  # strength 0: the frame without shadows, bit for bit (k = 1 either way)
            plain = SH.restate_case(lib, O, c, shadows=None)[0]
            assert dark.any() and (plain.view(np.uint32) == img.view(np.uint32)).all(), c
        if c.name == "strength 1":
            assert dark.any() and (~dark & hit).any(), c
    print("\nshadow fuzz cases, pixels of each kind on the restatement: " + ", ".join(f"{k.rstrip('_')} {v}" for k, v in n.items()))
    for k, v in n.items():
        assert v > 0, k
    # the clip box that removes the caster: pixels shadowed by the other ball without the box are lit with it
    with_box = next(c for c in cases if c.name == "caster clipped away")
    without = next(c for c in cases if c.name == "caster and receiver")
    (_, _, _, fb, _, nb), (_, _, _, fw, _, nw) = restated[cases.index(with_box)], restated[cases.index(without)]
    freed = ((fw & SH.SHADOWED) != 0) & (nw > 0) & ((fb & SH.HIT) != 0) & ((fb & SH.SHADOWED) == 0) & (nb > 0)
    print(f"caster clipped away: {int(freed.sum())} pixels shadowed without the box and lit with it")
    assert freed.sum() >= 20


def test_mask_cases_hold_few_pixels_without_a_diffuse_term(O, restated):
    """In a mask case a shadowed pixel is exactly 0 and an unshadowed one srgb(diff): pixels whose diff is 0 say nothing and are excluded
    by the GPU test; they are at most 1 % of each such case's hit pixels."""
    seen = 0
    for c, (img, steps, a, fl, iters, nl) in zip(shadow_cases.cases(O), restated):
        if not c.mask:
            continue
        hit, dark = (fl & SH.HIT) != 0, (fl & SH.SHADOWED) != 0
        flat = hit & (nl == 0)
        assert flat.sum() <= 0.01 * hit.sum(), (c, int(flat.sum()), int(hit.sum()))
        black = (img[..., :3] == 0).all(axis=2)
        assert (black[hit & ~flat] == dark[hit & ~flat]).all(), c  # the restatement's own frame shows its mask
        seen += int(hit.sum() > 0)
    assert seen >= 8


def test_numpy_reference_agrees_with_the_c_restatement(O, restated, referenced):
    worst = (0.0, None)
    for c, (img, ref_steps, ref_a, fl, ref_iters, _), (got, steps, _, hit, a, dark, iters) in zip(shadow_cases.cases(O), restated, referenced):
        ref = img[..., :3]
        assert np.isfinite(ref).all(), c  # no pixel is excluded below
        assert (steps == ref_steps).all(), (c, int((steps != ref_steps).sum()))
        assert (hit == ((fl & SH.HIT) != 0)).all(), c
        assert (a.view(np.uint32) == ref_a.view(np.uint32)).all(), (c, int((a != ref_a).sum()))
        assert (dark == ((fl & SH.SHADOWED) != 0)).all(), (c, int((dark != ((fl & SH.SHADOWED) != 0)).sum()))
        assert (iters == ref_iters).all(), (c, int((iters != ref_iters).sum()))
        assert np.isfinite(got).all(), c
        err = float(rel_err(got, ref).max())
        print(f"{c.name}: colour error {err:.3g}, {int(hit.sum())} hits, {int(dark.sum())} shadowed, {int(iters.sum())} shadow iterations")
        assert err <= TOL_LIT, (c, err)
        if err >= worst[0]:
            worst = (err, c.name)
        assert ref_steps.max() > 0, c  # every case marches something
    print(f"\nnumpy shadow reference vs C restatement, largest colour error {worst[0]:.3g} ({worst[1]})")


def test_numpy_reference_tile_is_the_frame_cropped(O, referenced):
    for c, full in ((c, r) for c, r in zip(shadow_cases.cases(O), referenced) if c.tile is not None):
        part = NS.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, iso=c.iso, colour=c.colour, refine=c.refine, dt=c.dt, light=c.light, shadow=c.shadows,
                         box=c.box, tile=c.tile)
        m = tile_mask(c)
        for p, f in zip(part, full):
            assert (p[m] == f[m]).all() and (p[~m] == 0).all()
        assert full[1][m].max() > 0 and full[5][m].any()
