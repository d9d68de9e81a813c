"""The two references of the slice pass (vk_render_slice) held together over the shared cases
(tests/slice_cases.py): the C restatement (tests/slice_restatement.c: f32, the specification's operation order, on the oracle's pieces)
and the numpy reference (tests/np_slice_reference.py: positions and taps from the dense array, the filter and the reductions in f32 with
numpy operations).

On EVERY pixel: P, inside and x are equal BIT FOR BIT (a NaN x is held to "is a NaN", geom_helpers.same_bits); colour agrees within the
unlit table kernels' bar, TOL_UNLIT, relative to max(1, |ref|).  The conditions on the case list -- one pixel at least of every kind -- are
asserted on the restatement's output, so the list cannot quietly degenerate.

The exact anchor involves no restatement: on a 16 x 8 x 4 volume under Slice.axial / coronal / sagittal at the volume's own size every
position is a texel centre exactly, so x must be the raw voxel as a float at every pixel, and a MEAN over an odd number of planes
f32(sum) * rn."""
import numpy as np
import pytest

import np_slice_reference as NS
import slice_cases
import slice_helpers as SH
from np_table_reference import srgb64
from test_table_fuzz_cpu import TOL_UNLIT


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("slice_fuzz_cpu"), O)


@pytest.fixture(scope="module")
def restated(O, lib):
    return [SH.restate_case(lib, c) for c in slice_cases.cases(O)]


def test_case_list_covers_the_edges(O):
    cases = slice_cases.cases(O)
    assert len(cases) == slice_cases.N_RANDOM + slice_cases.N_NAMED and slice_cases.N_RANDOM == 40
    assert {c.kind for c in cases} == {"u8", "f16", "u16"}
    assert max(max(c.dims) for c in cases) <= 24 and all(c.W <= 48 and c.H <= 32 for c in cases)
    for red in slice_cases.REDUCE:
        assert {c.samples for c in cases if c.reduce == red and c.samples > 1} >= {2, 3, 8, 256}, red
    assert any(c.samples == 1 for c in cases)
    for kind in ("u8", "f16", "u16"):
        assert any(c.kind == kind and c.table is None for c in cases) and any(c.kind == kind and c.table is not None for c in cases), kind
        assert any(c.kind == kind and c.samples > 1 for c in cases), kind
    assert any(c.box is not None for c in cases)
    assert any(c.tile is not None and min(c.tile[:2]) < 0 for c in cases) and any(c.tile is not None and min(c.tile[:2]) > 0 for c in cases)
    assert any(not c.plane[1].any() for c in cases) and any(not c.plane[2].any() for c in cases)  # du = 0, dv = 0
    assert sum(c.half for c in cases) >= 3
    assert {"oblique", "axis", "miss", "du zero", "dv zero"} <= {t for c in cases for t in c.tags}
    names = {c.name for c in cases}
    assert len(names) == len(cases)
    for n in ("1x1x1", "on the face z = 0", "on the face z = 1", "one ulp outside, below 0", "one ulp outside, above 1", "f16 NaN and inf taps, max",
              "f16 NaN and inf taps, min", "f16 NaN and inf taps, mean", "all-NaN slab, max", "all-NaN slab, min", "all-NaN slab, mean",
              "every slab sample clamps", "-0 table entries", "rgba16f u16 slab"):
        assert n in names, n


def test_case_list_conditions_hold_on_the_restatement(O, restated):
    cases = slice_cases.cases(O)
    n = dict(inside=0, outside=0, face=0, clamped=0, nan_passed=0, all_nan=0, mean_rounded=0)
    for c, (rgba, val, pos, fl) in zip(cases, restated):
        ins = (fl & SH.INSIDE) != 0
        assert (val[..., 1] == ins).all(), c                                          # the weight is the inside mask
        assert (rgba[~ins] == SH.CLEAR).all() and (val[~ins].view(np.uint32) == 0).all(), c  # the clear colour and the (+0, 0) record
        assert (rgba[..., 3] == 1.0).all(), c
        n["inside"] += int(ins.sum())
        n["outside"] += int((~ins).sum())
        n["face"] += int(((fl & SH.FACE) != 0).sum())
        n["clamped"] += int(((fl & SH.CLAMPED) != 0).sum())
        n["nan_passed"] += int(((fl & SH.NAN_PASSED) != 0).sum())
        n["all_nan"] += int(((fl & SH.ALL_NAN) != 0).sum())
        n["mean_rounded"] += int(((fl & SH.MEAN_ROUNDED) != 0).sum())
        if "face" in c.tags:
            assert ins.all() and ((fl & SH.FACE) != 0).all(), c
            z = 0.0 if c.name.endswith("0") else 1.0
            assert (pos[..., 2] == z).all() and pos[0, 0, 0] == 0.0 and pos[-1, -1, 0] == 1.0 and pos[-1, -1, 1] == 1.0, c
        if "ulp" in c.tags:
            assert not ins.any(), c
        if "miss" in c.tags:
            assert not ins.any(), c
        if "clamps" in c.tags:
            assert ins.all() and ((fl & SH.CLAMPED) != 0).all(), c
        if "allnan" in c.tags:
            assert ins.any(), c
            t = np.asarray(c.table, np.float64)
            want = {"max": (-np.inf, t[0, :3]), "min": (np.inf, t[-1, :3]), "mean": (None, t[0, :3])}[c.reduce]
            if c.reduce != "mean":
                assert (val[ins][:, 0] == want[0]).all() and ((fl[ins] & SH.ALL_NAN) != 0).all(), c
            else:
                assert np.isnan(val[ins][:, 0]).all(), c
            assert SH.rel_err(rgba[ins][:, :3], np.broadcast_to(srgb64(want[1]), rgba[ins][:, :3].shape)).max() <= TOL_UNLIT, c
        if c.name == "1x1x1":
            assert ins.any() and (val[ins][:, 0] == 200.0).all(), c
    print("\nslice cases, pixels of each kind on the restatement: " + ", ".join(f"{k} {v}" for k, v in n.items()))
    for k, v in n.items():
        assert v > 0, k


def test_numpy_reference_agrees_with_the_c_restatement(O, restated):
    worst = (0.0, None)
    for c, (rgba, val, pos, fl) in zip(slice_cases.cases(O), restated):
        rgb, nval, npos, ins = NS.render(c.vol, c.W, c.H, c.plane, samples=c.samples, reduce=c.reduce, table=c.table, domain=c.domain, box=c.box)
        assert (npos.view(np.uint32) == pos.view(np.uint32)).all(), (c, int((npos.view(np.uint32) != pos.view(np.uint32)).sum()))
        assert (ins == ((fl & SH.INSIDE) != 0)).all(), c
        same = SH.same_bits(nval, val)
        assert same.all(), (c, int((~same).sum()))
        assert np.isfinite(rgba).all(), c
        err = float(SH.rel_err(rgb, rgba[..., :3]).max())
        assert err <= TOL_UNLIT, (c, err)
        if err >= worst[0]:
            worst = (err, c.name)
    print(f"\nnumpy slice reference vs C restatement: P, inside and x bit for bit; the largest colour error is {worst[0]:.3g} ({worst[1]})")


def test_numpy_reference_tile_is_the_frame_cropped(O, lib, restated):
    seen = 0
    for c, (rgba, val, pos, fl) in ((c, r) for c, r in zip(slice_cases.cases(O), restated) if c.tile is not None):
        m = SH.tile_mask(c)
        rgb, nval, npos, ins = NS.render(c.vol, c.W, c.H, c.plane, samples=c.samples, reduce=c.reduce, table=c.table, domain=c.domain, box=c.box, tile=c.tile)
        assert SH.same_bits(nval[m], val[m]).all() and (nval[~m].view(np.uint32) == 0).all() and not ins[~m].any(), c
        t_rgba, t_val, _, _ = SH.restate_case(lib, c, tile=True)
        assert SH.same_bits(t_val[m], val[m]).all() and (t_val[~m].view(np.uint32) == 0).all(), c
        assert (t_rgba[m] == rgba[m]).all() and (t_rgba[~m] == SH.CLEAR).all(), c
        seen += 1
    assert seen >= 10


# ---- the exact anchor: no restatement involved ----

ANCHOR_DIMS = (16, 8, 4)  # nx, ny, nz: powers of two, so (i + 0.5) / n and the fmas are exact


def anchor_volumes():
    rng = np.random.default_rng(77)
    nx, ny, nz = ANCHOR_DIMS
    return {"u8": rng.integers(0, 256, (nz, ny, nx)).astype(np.uint8), "u16": rng.integers(0, 65536, (nz, ny, nx)).astype(np.uint16),
            "f16": rng.uniform(-2.0, 2.0, (nz, ny, nx)).astype(np.float16)}


def anchor_views(V):
    """(name, slice builder, frame size, the voxel plane of index k as [H, W], the axis the slab runs along)."""
    nx, ny, nz = ANCHOR_DIMS
    return (("axial", V.Slice.axial, (nx, ny), lambda vol, k: vol[k, :, :], 0, nz),
            ("coronal", V.Slice.coronal, (nx, nz), lambda vol, k: vol[:, k, :], 1, ny),
            ("sagittal", V.Slice.sagittal, (ny, nz), lambda vol, k: vol[:, :, k], 2, nx))


def anchor_expected_mean(vol, plane_of, k, samples, n_axis):
    """f32(sum) * rn over the planes k - (samples - 1) / 2 .. k + (samples - 1) / 2, indices clamped to the edge, summed in that order in f32."""
    acc = np.zeros(plane_of(vol, 0).shape, np.float32)
    for j in range(samples):
        acc = (acc + plane_of(vol, min(max(k + j - (samples - 1) // 2, 0), n_axis - 1)).astype(np.float32)).astype(np.float32)
    return (acc * np.float32(1.0 / samples)).astype(np.float32)


def plane_of_vk(s):
    return np.array([s.origin[:], s.du[:], s.dv[:], s.dn[:]], np.float32)


def test_exact_anchor_on_the_numpy_reference():
    import vokselis_amd as V

    checked = 0
    for kind, vol in anchor_volumes().items():
        for name, build, (W, H), plane_of, _, n_axis in anchor_views(V):
            for k in range(n_axis):
                s = build(ANCHOR_DIMS, k, W, H)
                _, val, _, ins = NS.render(vol, W, H, plane_of_vk(s))
                assert ins.all(), (kind, name, k)
                assert (val[..., 0].view(np.uint32) == plane_of(vol, k).astype(np.float32).view(np.uint32)).all(), (kind, name, k)
                checked += 1
            for samples in (3, 5):
                k = n_axis // 2
                s = build(ANCHOR_DIMS, k, W, H, samples=samples, reduce="mean")
                _, val, _, ins = NS.render(vol, W, H, plane_of_vk(s), samples=samples, reduce="mean")
                want = anchor_expected_mean(vol, plane_of, k, samples, n_axis)
                assert ins.all() and (val[..., 0].view(np.uint32) == want.view(np.uint32)).all(), (kind, name, samples)
                checked += 1
    assert checked == 3 * (4 + 8 + 16 + 6)
