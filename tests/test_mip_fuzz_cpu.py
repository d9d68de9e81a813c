"""The two references of the maximum-intensity projection held together over the shared fuzz cases (tests/mip_cases.py): the C restatement
(tests/mip_restatement.c: f32, the specification's operation order) and the numpy reference (tests/np_mip_reference.py: the maximum exact,
the lookup and sRGB in float64).

Step counts must be equal at every pixel.  Colour must agree within the bar tests/test_table_fuzz_cpu.py holds the unlit table lookup to
(2e-5 relative to max(1, |ref|): a float64 lookup against an f32 one) on EVERY pixel: the restatement's output is asserted finite first.
The conditions on the case list are asserted on the restatement, so the list cannot quietly degenerate."""
import numpy as np
import pytest

import mip_cases
import mip_helpers as MH
import np_mip_reference as NM
from test_table_fuzz_cpu import TOL_UNLIT, rel_err, tile_mask

TOL = TOL_UNLIT


@pytest.fixture(scope="module")
def lib(O, tmp_path_factory):
    return MH.build_restatement(tmp_path_factory.mktemp("mip_fuzz_cpu"), O)


@pytest.fixture(scope="module")
def restated(O, lib):
    return [MH.restate_case(lib, O, c) for c in mip_cases.cases(O)]


def test_case_list_covers_the_edges(O):
    cases = mip_cases.cases(O)
    assert len(cases) == mip_cases.N_CASES
    assert {c.dt for c in cases} == set(mip_cases.DTS)
    assert {c.table.shape[0] for c in cases if c.table is not None} == {2, 3, 17, 256}
    assert sum(c.table is None for c in cases) >= 4
    for f16 in (False, True):
        assert any(c.f16 == f16 and c.dt == 0.5 for c in cases)
    for dims in mip_cases.FIXED_DIMS:
        assert any(c.dims == dims for c in cases), dims
    assert any(c.tile is not None and min(c.tile[:2]) < 0 for c in cases)
    assert {c.empty for c in cases} >= {0.0, 1.0, None}
    assert any(c.half and c.f16 for c in cases) and any(c.half and not c.f16 for c in cases)
    assert any(c.table is not None and np.abs(c.table[:, :3]).max() == np.float32(1e30) for c in cases)
    assert any(c.table is not None and np.signbit(c.table[0, :3]).all() and (c.table[0, :3] == 0).all() for c in cases)  # T[0] = -0
    for kind in set(mip_cases.WINDOWS):
        assert any(kind in c.tags for c in cases), kind
    bits = np.concatenate([c.vol.view(np.uint16).ravel() for c in cases if c.f16])
    for b in mip_cases.TC.F16_NAN_BITS + (0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x8001):  # NaNs, +-inf, +-0, subnormals
        assert (bits == b).any(), hex(b)
    u8 = np.concatenate([c.vol.ravel() for c in cases if not c.f16])
    assert (u8 == 0).any() and (u8 == 255).any()


def test_case_list_conditions_hold_on_the_restatement(O, restated):
    """Rays that end by the break and rays that never do, a maximum in the very last iteration, NaN samples ignored, +inf samples saturating."""
    cases = mip_cases.cases(O)
    broke_share, sizes = [], set()
    last = nan_ignored = inf_saturates = False
    for c, (img, steps, U, fl) in zip(cases, restated):
        hit = (fl & MH.HIT) != 0
        ran = hit & (steps > 0)
        if ran.any():
            broke_share.append(float(((fl & MH.BROKE) != 0)[ran].mean()))
            sizes.add(c.n if c.table is not None else None)
        last |= bool(((fl & MH.MAX_AT_LAST) != 0).any())
        # a NaN sample was seen and the ray neither saturated nor ended up NaN: it was ignored (U is finite by construction of tf_u)
        nan_ignored |= bool((((fl & MH.NAN_SEEN) != 0) & ((fl & MH.BROKE) == 0) & (U > 0) & (U < c.n - 1)).any())
        inf_saturates |= bool((((fl & MH.PINF_SEEN) != 0) & ((fl & MH.BROKE) != 0)).any())
        assert np.isfinite(U).all() and (U >= 0).all() and (U <= c.n - 1).all() and not np.signbit(U).any(), c
    assert max(broke_share) > 0.1 and min(broke_share) == 0.0, (max(broke_share), min(broke_share))
    assert sum(s > 0.1 for s in broke_share) >= 5 and sum(s == 0.0 for s in broke_share) >= 5
    assert last, "no ray whose maximum comes from its last iteration"
    assert nan_ignored, "no ray that saw a NaN sample and ignored it"
    assert inf_saturates, "no ray saturated by a +inf sample"
    assert sizes >= {2, 3, 17, 256, None}


def test_numpy_reference_agrees_with_the_c_restatement(O, restated):
    worst = (0.0, None)
    for c, (img, ref_steps, U, fl) in zip(mip_cases.cases(O), restated):
        ref = img[..., :3]
        assert np.isfinite(ref).all(), c  # no pixel is excluded below
        got, steps, _ = NM.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt)
        assert (steps == ref_steps).all(), (c, int((steps != ref_steps).sum()))
        assert np.isfinite(got).all(), c
        err = float(rel_err(got, ref).max())
        assert err <= TOL, (c, err)
        if err >= worst[0]:
            worst = (err, c.name)
        assert ref_steps.max() > 0, c  # every case marches something
    print(f"\nnumpy MIP reference vs C restatement, largest colour error {worst[0]:.3g} ({worst[1]})")


def test_numpy_reference_tile_is_the_frame_cropped(O):
    for c in (c for c in mip_cases.cases(O) if c.tile is not None):
        cam = O.camera_blob(*c.cam)
        full, fsteps, flive = NM.render(cam, c.vol, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt)
        part, psteps, plive = NM.render(cam, c.vol, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt, tile=c.tile)
        m = tile_mask(c)
        assert (part[m] == full[m]).all() and (psteps[m] == fsteps[m]).all() and (plive[m] == flive[m]).all() and fsteps[m].max() > 0
        assert (part[~m] == 0).all() and (psteps[~m] == 0).all()


def test_empty_fraction_cases_count_as_built(O):
    """The reference's count of iterations in non-empty cells is 0 where every cell is empty and the step count where none is."""
    for c in (c for c in mip_cases.cases(O) if c.empty is not None):
        _, steps, live = NM.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt)
        assert steps.sum() > 0
        assert int(live.sum()) == (0 if c.empty == 1.0 else int(steps.sum())), c


def test_raising_a_voxel_never_lowers_a_pixel(O, lib):
    """Needs no reference: under the grey ramp, raising one voxel of a u8 volume never lowers any pixel's U."""
    rng = np.random.default_rng(7)
    cam = O.camera_blob(1.3, 0.4, 0.9, (0.5, 0.5, 0.5), 1.0)
    vol = rng.integers(0, 200, (9, 11, 10)).astype(np.uint8)
    _, _, U0, _ = MH.restate(lib, O, cam, vol, 40, 40, dt=0.5)
    raised = 0
    for _ in range(12):
        z, y, x = (int(rng.integers(0, s)) for s in vol.shape)
        v2 = vol.copy()
        v2[z, y, x] = min(255, int(vol[z, y, x]) + int(rng.integers(1, 120)))
        _, _, U1, _ = MH.restate(lib, O, cam, v2, 40, 40, dt=0.5)
        assert (U1 >= U0).all()
        raised += int((U1 > U0).any())
    assert raised >= 3  # (a raise hidden behind a brighter neighbour changes nothing: most are not)


@pytest.mark.parametrize("v", [0, 1, 77, 128, 254, 255])
def test_constant_volume_shows_the_table_at_its_value(O, lib, v):
    """The MIP of a constant volume v inside the window is T(u(v)) on every hit ray with at least one iteration."""
    rng = np.random.default_rng(v)
    table = mip_cases.TC.random_table(rng, 17)
    cam = O.camera_blob(1.3, 0.4, 0.9, (0.5, 0.5, 0.5), 1.0)
    img, steps, U, fl = MH.restate(lib, O, cam, np.full((6, 7, 8), v, np.uint8), 32, 32, dt=0.7, table=table, domain=(0.0, 1.0))
    ran = steps > 0
    assert ran.any()
    k1, k2 = MH.tf_constants(17, np.float32(0.0), np.float32(1.0), True)
    u = min(max(float(np.float32(np.float64(v) * np.float64(np.float32(k1)) + np.float64(np.float32(k2)))), 0.0), 16.0)
    assert (U[ran] == np.float32(u)).all()
    i = min(int(np.floor(u)), 15)
    want = NM.srgb64(table[i, :3].astype(np.float64) + (u - i) * (table[i + 1, :3].astype(np.float64) - table[i, :3].astype(np.float64)))
    assert rel_err(img[ran][:, :3], np.broadcast_to(want, img[ran][:, :3].shape)).max() <= TOL
