"""The two references of the geometry pass of the first-hit isosurface (vk_render_geometry) held together over the
shared cases (tests/geom_cases.py): the C restatement (tests/geom_restatement.c: f32, the specification's operation order) and the numpy
reference (tests/np_geom_reference.py: hit mask, a, q, t and x exact in f32, the gradient in float64 from the eight taps).

On EVERY pixel: the hit mask, a, q, t and x are equal; g agrees within a derived bar.  g is a handful of f32 roundings of differences of
taps, times a dimension: per component the bar is 16 * 2^-24 * max|tap| * max(n), with max|tap| the largest finite tap of the case's
volume on the kernel's scale and n its dimensions.  The largest error seen is printed as a share of the bar.  Where the float64 gradient is
not finite (a cell with an infinite or NaN tap) the restatement's must not be finite either.
The conditions on the case list -- one pixel at least of every kind of ray -- are asserted on the restatement, so the list cannot quietly
degenerate.  And the restatement's colour-independent outputs (steps, hit mask, a) equal tests/iso_restatement.c's on the cases the two
share: the pass is the colour render's ray."""
import numpy as np
import pytest

import geom_cases
import geom_helpers as GH
import iso_cases
import iso_helpers as IH
import np_geom_reference as NG


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return GH.build_restatement(tmp_path_factory.mktemp("geom_fuzz_cpu"), O)


@pytest.fixture(scope="module")
def restated(O, lib):
    return [GH.restate_case(lib, O, c) for c in geom_cases.cases(O)]


def g_bar(c):
    v = c.vol.astype(np.float32)
    return 16.0 * 2.0 ** -24 * float(np.abs(v[np.isfinite(v)]).max(initial=0.0)) * max(c.dims)


def test_case_list_covers_the_edges(O):
    cases = geom_cases.cases(O)
    assert {c.kind for c in cases} == {"u8", "f16", "u16"}
    for kind in ("u8", "f16", "u16"):
        assert any(c.kind == kind and c.box is not None for c in cases), kind
        assert any(c.kind == kind and c.light is None for c in cases) and any(c.kind == kind and c.light is not None for c in cases), kind
    assert {c.refine for c in cases} >= {0, 1, 4, 16}
    assert any(c.dims == (1, 1, 1) for c in cases)
    assert any(c.tile is not None and min(c.tile[:2]) < 0 for c in cases) and any(c.tile is not None and min(c.tile[:2]) > 0 for c in cases)
    assert max(max(c.dims) for c in cases) <= 65 and all(24 <= min(c.W, c.H) and max(c.W, c.H) <= 80 for c in cases)
    names = {c.name for c in cases}
    assert len(names) == len(cases)
    for n in ("1x1x1", "tile at a negative origin, clip box", "first-iteration hits on a clip face", "R = 0", "R = 16", "iso above all data", "+inf tap hit",
              "NaN samples passed over"):
        assert n in names, n


def test_case_list_conditions_hold_on_the_restatement(O, restated):
    cases = geom_cases.cases(O)
    n = dict(first=0, later_zero=0, later_mid=0, later_top=0, never=0, box_miss=0, no_gradient=0, clip_face=0, nan_passed=0, pinf=0)
    for c, (rec, steps, a, fl) in zip(cases, restated):
        box, hit, fst = (fl & GH.BOX) != 0, (fl & GH.HIT) != 0, (fl & GH.FIRST) != 0
        later = hit & ~fst
        top = np.float32(1.0 - 2.0 ** -c.refine)
        t = rec[:, :, 0, 3]
        assert (np.isfinite(t) == hit).all(), c                       # isfinite(t) is the hit mask
        assert GH.same_bits(rec[~hit], GH.MISS).all(), c              # every other pixel holds the miss record
        assert np.isfinite(rec[hit][:, 0, :]).all() and (t[hit] >= 0).all(), c
        assert (a[fst] == 0).all() and (a >= 0).all() and (a <= top).all() and (a[~hit] == 0).all(), c
        n["first"] += int(fst.sum())
        n["never"] += int((box & ~hit & (steps > 0)).sum())
        n["box_miss"] += int((~box).sum())
        if c.refine > 0:
            n["later_zero"] += int((later & (a == 0)).sum())
            n["later_mid"] += int((later & (a > 0) & (a < top)).sum())
            n["later_top"] += int((later & (a == top)).sum())
        n["no_gradient"] += int((hit & (rec[:, :, 1, :3] == 0).all(axis=2)).sum())
        if c.box is not None:  # a first-iteration hit whose q lies on a face of the clip box inside the unit cube
            q = rec[:, :, 0, :3]
            on = np.zeros(hit.shape, bool)
            for k in range(3):
                for b in (c.box[0][k], c.box[1][k]):
                    if 0.0 < b < 1.0:
                        on |= np.abs(q[..., k] - np.float32(b)) <= 1e-5
            n["clip_face"] += int((fst & on).sum())
        n["nan_passed"] += int((((fl & GH.NAN_SEEN) != 0) & hit & (steps >= 2)).sum())
        n["pinf"] += int(((fl & GH.PINF_HIT) != 0).sum())
        if c.name == "iso above all data":
            assert not hit.any() and steps.max() > 1 and GH.same_bits(rec, GH.MISS).all(), c
        if c.name == "first-iteration hits on a clip face":
            assert hit.sum() > 100 and fst[hit].all(), c
        if c.name == "1x1x1":
            assert hit.any() and fst[hit].all() and (rec[hit][:, 1, :3] == 0).all() and (rec[hit][:, 1, 3] == 200.0).all(), c
        if c.name == "+inf tap hit":
            assert ((fl & GH.PINF_HIT) != 0).sum() > 20, c
        if c.name == "NaN samples passed over":
            assert (((fl & GH.NAN_SEEN) != 0) & hit).sum() > 20, c
    print("\ngeometry cases, pixels of each kind on the restatement: " + ", ".join(f"{k} {v}" for k, v in n.items()))
    for k, v in n.items():
        assert v > 0, k


def test_numpy_reference_agrees_with_the_c_restatement(O, restated):
    worst = (0.0, None)
    for c, (rec, ref_steps, ref_a, fl) in zip(geom_cases.cases(O), restated):
        pos_t, g, x, hit, a, steps = NG.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, iso=c.iso, refine=c.refine, dt=c.dt, box=c.box)
        assert (steps == ref_steps).all(), (c, int((steps != ref_steps).sum()))
        assert (hit == ((fl & GH.HIT) != 0)).all(), c
        assert (a.view(np.uint32) == ref_a.view(np.uint32)).all(), (c, int((a != ref_a).sum()))
        assert (pos_t.view(np.uint32) == rec[:, :, 0, :].view(np.uint32)).all(), (c, int((pos_t.view(np.uint32) != rec[:, :, 0, :].view(np.uint32)).sum()))
        assert GH.same_bits(x, rec[:, :, 1, 3]).all(), c
        got = rec[:, :, 1, :3].astype(np.float64)
        fin = np.isfinite(g)
        assert not np.isfinite(got[~fin]).any(), c
        bar = g_bar(c)
        err = float(np.abs(got[fin] - g[fin]).max(initial=0.0))
        share = err / bar if bar > 0 else 0.0
        print(f"{c.name}: {int(hit.sum())} hits, gradient error {err:.3g}, bar {bar:.3g} ({share:.2%} of it)")
        assert err <= bar, (c, err, bar)
        if share >= worst[0]:
            worst = (share, c.name)
    print(f"\nnumpy geometry reference vs C restatement: the largest gradient error is {worst[0]:.2%} of its bar ({worst[1]})")


def test_numpy_reference_tile_is_the_frame_cropped(O, restated):
    for c, (rec, _, _, _) in ((c, r) for c, r in zip(geom_cases.cases(O), restated) if c.tile is not None):
        pos_t, g, x, hit, a, steps = NG.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, iso=c.iso, refine=c.refine, dt=c.dt, box=c.box, tile=c.tile)
        m = GH.tile_mask(c)
        assert (pos_t[m].view(np.uint32) == rec[:, :, 0, :][m].view(np.uint32)).all(), c
        assert GH.same_bits(pos_t[~m], GH.MISS[0]).all() and not hit[~m].any() and hit[m].any(), c


def test_the_pass_is_the_colour_renders_ray(O, lib, restated, tmp_path_factory):
    """Steps, hit mask and a of tests/iso_restatement.c on the shared cases, whatever their lighting."""
    iso_lib = IH.build_restatement(tmp_path_factory.mktemp("geom_iso_cpu"), O)
    by_name = {c.name: r for c, r in zip(geom_cases.cases(O), restated)}
    seen = 0
    for c in iso_cases.cases(O):
        _, steps, a, fl = IH.restate_case(iso_lib, O, c)
        rec, gsteps, ga, gfl = by_name["iso " + c.name]
        assert (steps == gsteps).all() and (a.view(np.uint32) == ga.view(np.uint32)).all(), c
        assert (((fl & IH.HIT) != 0) == ((gfl & GH.HIT) != 0)).all() and (((fl & IH.FIRST) != 0) == ((gfl & GH.FIRST) != 0)).all(), c
        seen += 1
    assert seen == iso_cases.N_CASES
