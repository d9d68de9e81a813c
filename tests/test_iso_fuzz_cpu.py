"""The two references of first-hit isosurface rendering held together over the shared fuzz cases (tests/iso_cases.py): the C restatement
(tests/iso_restatement.c: f32, the specification's operation order) and the numpy reference (tests/np_iso_reference.py: the hit test and
the bisection exact in f32, the shade and sRGB in float64).

Step counts, the hit mask and the refined a must be equal at every pixel.  Colour must agree within the bars tests/test_table_fuzz_cpu.py
holds the table march to -- the shade is the same lit_shade, evaluated once per ray instead of accumulated: TOL_UNLIT = 2e-5 unlit and
TOL_LIT = 1e-4 lit, relative to max(1, |ref|), on EVERY pixel: the restatement's output is asserted finite first.  The conditions on the
case list are asserted on the restatement, so the list cannot quietly degenerate."""
import numpy as np
import pytest

import iso_cases
import iso_helpers as IH
import np_iso_reference as NI
from test_table_fuzz_cpu import TOL_LIT, TOL_UNLIT, rel_err, tile_mask


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return IH.build_restatement(tmp_path_factory.mktemp("iso_fuzz_cpu"), O)


@pytest.fixture(scope="module")
def restated(O, lib):
    return [IH.restate_case(lib, O, c) for c in iso_cases.cases(O)]


@pytest.fixture(scope="module")
def referenced(O):
    return [NI.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, iso=c.iso, colour=c.colour, refine=c.refine, dt=c.dt, light=c.light)
            for c in iso_cases.cases(O)]


def test_case_list_covers_the_edges(O):
    cases = iso_cases.cases(O)
    assert len(cases) == iso_cases.N_CASES
    assert {c.dt for c in cases} == set(iso_cases.DTS)
    assert {c.refine for c in cases} == {0, 1, 4, 16}
    for f16 in (False, True):
        assert any(c.f16 == f16 and c.dt == 0.5 for c in cases)
    for dims in iso_cases.FIXED_DIMS:
        assert any(c.dims == dims for c in cases), dims
    assert max(max(c.dims) for c in cases) <= 65 and all(24 <= min(c.W, c.H) and max(c.W, c.H) <= 80 for c in cases)
    assert any(c.tile is not None and min(c.tile[:2]) < 0 for c in cases)
    assert any(c.tile is not None and min(c.tile[:2]) > 0 and c.tile[0] + c.tile[2] < c.W and c.tile[1] + c.tile[3] < c.H for c in cases)
    assert {c.empty for c in cases} >= {0.0, 1.0, None}
    assert any(c.half and c.f16 for c in cases) and any(c.half and not c.f16 for c in cases)
    # lights: none, headlight, fixed, random; every coefficient at 16 with shininess 1 and with shininess 1024
    assert any(c.light is None for c in cases) and any(c.light and c.light["direction"] == "headlight" for c in cases)
    assert any(c.light and c.light["direction"] == (1.0, 0.0, 0.0) for c in cases)
    for kind in set(iso_cases.LIGHTS):
        assert any(kind in c.tags for c in cases), kind
    for n in (1.0, 1024.0):
        assert any(c.light and (c.light["ambient"], c.light["diffuse"], c.light["specular"], c.light["shininess"]) == (16.0, 16.0, 16.0, n) for c in cases), n
    assert any(max(abs(v) for v in c.colour) == 1e30 for c in cases)
    assert any(not c.f16 and IH.iso_k(c.iso, True) == -np.inf for c in cases) and any(not c.f16 and IH.iso_k(c.iso, True) == np.inf for c in cases)
    assert any(c.iso == 1.0 and not c.f16 and IH.iso_k(c.iso, True) == np.float32(255.0) and (c.vol == 255).any() for c in cases)
    bits = np.concatenate([c.vol.view(np.uint16).ravel() for c in cases if c.f16])
    for b in iso_cases.TC.F16_NAN_BITS + (0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x8001):  # NaNs, +-inf, +-0, subnormals
        assert (bits == b).any(), hex(b)


def test_case_list_conditions_hold_on_the_restatement(O, restated):
    """Hits in the first iteration (unrefined), later hits with a = 0, 0 < a < 1 - 2^-R and a = 1 - 2^-R, rays through the box that never
    hit, a hit by equality, NaN samples that are no hit, +inf samples that are one; thresholds below and above all data."""
    cases = iso_cases.cases(O)
    first = later_zero = later_mid = later_top = never = equal = nan_no_hit = pinf_hit = False
    refined_depths = set()
    for c, (img, steps, a, fl) in zip(cases, restated):
        box, hit, fst = (fl & IH.BOX) != 0, (fl & IH.HIT) != 0, (fl & IH.FIRST) != 0
        later = hit & ~fst
        top = np.float32(1.0 - 2.0 ** -c.refine)
        assert (a[fst] == 0).all() and (steps[fst] == 1).all() and (steps[later] >= 2).all(), c
        assert (a >= 0).all() and (a <= top).all() and (a[~hit] == 0).all(), c
        assert (np.ldexp(a.astype(np.float64), c.refine) % 1.0 == 0).all(), c  # a dyadic of R bits
        first |= bool(fst.any())
        never |= bool((box & ~hit & (steps > 0)).any())
        if c.refine > 0:
            later_zero |= bool((later & (a == 0)).any())
            later_mid |= bool((later & (a > 0) & (a < top)).any())
            later_top |= bool((later & (a == top)).any())
            if (later & (a > 0)).any():
                refined_depths.add(c.refine)
        else:
            assert (a == 0).all(), c
        equal |= bool(((fl & IH.EQUAL) != 0).any()) and c.iso == 1.0
        nan_no_hit |= bool((((fl & IH.NAN_SEEN) != 0) & (steps >= 2)).any())  # a NaN sample was seen and the loop went on past it, or ended without it hitting
        pinf_hit |= bool(((fl & IH.PINF_HIT) != 0).any())
        if c.empty == 0.0:  # below all data: every ray through the box hits at once
            assert (hit[box & (steps > 0)]).all() and (steps[box] <= 1).all() and fst[hit].all(), c
        if c.empty == 1.0:  # above all data: all background
            assert not hit.any() and (img == [0.0, 0.0, 0.0, 1.0]).all() and steps.max() > 1, c
    assert first and later_zero and later_mid and later_top and never, (first, later_zero, later_mid, later_top, never)
    assert refined_depths == {1, 4, 16}, refined_depths
    assert equal, "no hit by equality at iso_k == 255"
    assert nan_no_hit, "no ray that saw a NaN sample and went on"
    assert pinf_hit, "no ray stopped by a +inf sample"


def test_numpy_reference_agrees_with_the_c_restatement(O, restated, referenced):
    worst = {False: (0.0, None), True: (0.0, None)}
    for c, (img, ref_steps, ref_a, fl), (got, steps, _, hit, a) in zip(iso_cases.cases(O), restated, referenced):
        ref = img[..., :3]
        assert np.isfinite(ref).all(), c  # no pixel is excluded below
        assert (steps == ref_steps).all(), (c, int((steps != ref_steps).sum()))
        assert (hit == ((fl & IH.HIT) != 0)).all(), c
        assert (a.view(np.uint32) == ref_a.view(np.uint32)).all(), (c, int((a != ref_a).sum()))
        assert np.isfinite(got).all(), c
        lit = c.light is not None
        err = float(rel_err(got, ref).max())
        print(f"{c.name}: colour error {err:.3g} ({'lit' if lit else 'unlit'})")
        assert err <= (TOL_LIT if lit else TOL_UNLIT), (c, err)
        if err >= worst[lit][0]:
            worst[lit] = (err, c.name)
        assert ref_steps.max() > 0, c  # every case marches something
    print(f"\nnumpy isosurface reference vs C restatement, largest colour error unlit {worst[False][0]:.3g} ({worst[False][1]}), "
          f"lit {worst[True][0]:.3g} ({worst[True][1]})")


def test_numpy_reference_tile_is_the_frame_cropped(O, referenced):
    for c, full in ((c, r) for c, r in zip(iso_cases.cases(O), referenced) if c.tile is not None):
        part = NI.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, iso=c.iso, colour=c.colour, refine=c.refine, dt=c.dt, light=c.light, tile=c.tile)
        m = tile_mask(c)
        for p, f in zip(part, full):
            assert (p[m] == f[m]).all() and (p[~m] == 0).all()
        assert full[1][m].max() > 0


def test_empty_fraction_cases_count_as_built(O, referenced):
    """The reference's count of iterations in non-empty cells is 0 where every cell is empty and the step count where none is."""
    for c, (_, steps, live, _, _) in ((c, r) for c, r in zip(iso_cases.cases(O), referenced) if c.empty is not None):
        assert steps.sum() > 0
        assert int(live.sum()) == (0 if c.empty == 1.0 else int(steps.sum())), c


def test_a_hit_never_lies_in_an_empty_cell(O, referenced):
    """Needs no second reference: the iteration that hits is always one whose cell is not empty, so a ray that hit counts at least one."""
    for c, (_, steps, live, hit, _) in zip(iso_cases.cases(O), referenced):
        assert (live[hit] >= 1).all() and (live <= steps).all(), c


def test_unlit_frame_is_the_colour_wherever_the_ray_hit(O, lib):
    """Unlit, the frame is srgb(colour) on the hit mask and background elsewhere, whatever the refinement depth."""
    c = next(c for c in iso_cases.cases(O) if c.name == "tile inside")
    frames = [IH.restate(lib, O, O.camera_blob(*c.cam), c.vol, c.W, c.H, iso=c.iso, colour=c.colour, refine=r, dt=c.dt) for r in (0, 4, 16)]
    hit = (frames[0][3] & IH.HIT) != 0
    assert hit.any() and not hit.all()
    want = NI.srgb64(np.array(c.colour, np.float32).astype(np.float64))
    for img, steps, a, fl in frames:
        assert (img.view(np.uint32) == frames[0][0].view(np.uint32)).all() and (steps == frames[0][1]).all()
        assert rel_err(img[hit][:, :3], np.broadcast_to(want, img[hit][:, :3].shape)).max() <= TOL_UNLIT
        assert (img[~hit] == [0.0, 0.0, 0.0, 1.0]).all()
