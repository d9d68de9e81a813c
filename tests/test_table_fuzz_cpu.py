"""The two references of the table march and the lit table march held together over the shared fuzz cases (tests/table_cases.py): the
C restatements (tests/tf_restatement.c, tests/lit_restatement.c: f32, in the kernels' operation order) and the numpy reference
(tests/np_table_reference.py: the alpha chain in f32, everything that only moves colour in float64).

Step counts must be equal.  Colour must agree within 2e-5 per channel unlit and 1e-4 lit, relative to max(1, |ref|) (the tables with
colours near VK_TF_MAX_COLOUR reach ~1e12 after linear_to_srgb), at every dt_scale of the list, 0.013 included.  Both frames are finite
wherever the other is."""
import numpy as np
import pytest

import lit_helpers
import np_table_reference as NR
import table_cases
import tf_helpers

TOL_UNLIT, TOL_LIT = 2e-5, 1e-4


@pytest.fixture(scope="module")
def libs(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("table_fuzz_cpu")
    return tf_helpers.build_restatement(d, O), lit_helpers.build_restatement(d, O)


def light_vector(light):
    return lit_helpers.light_vector(light["direction"], light["ambient"], light["diffuse"], light["specular"], light["shininess"])


def restate(libs, O, c):
    """The C restatement's frame (rgb f32 [H, W, 3], steps) of a case over its whole frame: tf_restatement.c unlit, lit_restatement.c lit."""
    cam = O.camera_blob(*c.cam)
    if c.light is None:
        img, steps = tf_helpers.restate(libs[0], O, cam, c.vol, c.W, c.H, dt=c.dt, table=c.table, domain=c.domain)
    else:
        img, steps = lit_helpers.restate(libs[1], O, cam, c.vol, c.W, c.H, dt=c.dt, table=c.table, domain=c.domain, light=light_vector(c.light))
    return img[..., :3], steps


def rel_err(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.maximum(1.0, np.abs(ref.astype(np.float64)))


def test_case_list_covers_the_edges(O):
    """The list is the one the GPU fuzz walks; what it must hold does not depend on the draw."""
    cases = table_cases.cases(O)
    assert len(cases) == table_cases.N_CASES == 62
    assert {c.dt for c in cases} == set(table_cases.DTS)
    assert {c.table.shape[0] for c in cases} == {2, 3, 17, 256}
    for f16 in (False, True):  # dt 0.5 for every layout: u8 cases run on LINEAR, PACKED, PACKED_PAIRS; f16 cases on LINEAR, PACKED
        assert any(c.f16 == f16 and c.dt == 0.5 for c in cases)
        assert any(c.f16 == f16 and c.light is not None for c in cases) and any(c.f16 == f16 and c.light is None for c in cases)
    for dims in table_cases.FIXED_DIMS:
        assert any(c.dims == dims for c in cases), dims
    assert any(c.tile is not None and min(c.tile[:2]) < 0 for c in cases)
    assert {c.empty for c in cases} >= {0.0, 1.0, None}
    assert any(c.half and c.f16 and c.dt == 0.5 for c in cases) and any(c.half and not c.f16 and c.dt == 0.5 for c in cases)
    assert any(c.big and c.light is not None for c in cases) and any(c.big and c.light is None for c in cases)
    bits = np.concatenate([c.vol.view(np.uint16).ravel() for c in cases if c.f16])
    for b in table_cases.F16_NAN_BITS + (0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x8001):  # NaNs, +-inf, +-0, subnormals
        assert (bits == b).any(), hex(b)
    lights = [c.light for c in cases if c.light is not None]
    assert any(li["direction"] == "headlight" for li in lights)
    for axis in ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)):
        assert any(li["direction"] == axis for li in lights), axis
    for k, bounds in (("ambient", (0.0, 16.0)), ("diffuse", (0.0, 16.0)), ("specular", (0.0, 16.0)), ("shininess", (1.0, 1024.0))):
        assert {li[k] for li in lights} >= set(bounds), k
    assert any((c.table[:, 3] == 0).any() and np.signbit(c.table[:, 3][c.table[:, 3] == 0]).any() for c in cases)  # alpha -0.0
    assert any((c.table[:, 3] == 1.0).any() for c in cases)


def test_numpy_reference_agrees_with_the_c_restatements(O, libs):
    worst = {"unlit": (0.0, None), "lit": (0.0, None)}
    shown = 0
    for c in table_cases.cases(O):
        ref, ref_steps = restate(libs, O, c)
        got, steps = NR.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt, light=c.light)
        assert (steps == ref_steps).all(), (c, int((steps != ref_steps).sum()))
        assert (np.isfinite(got) == np.isfinite(ref)).all(), c
        fin = np.isfinite(ref)
        err = float(rel_err(got[fin], ref[fin]).max()) if fin.any() else 0.0
        kind = "unlit" if c.light is None else "lit"
        assert err <= (TOL_UNLIT if c.light is None else TOL_LIT), (c, err)
        if err >= worst[kind][0]:
            worst[kind] = (err, c.name)
        shown += int(ref_steps.max() > 0)
    assert shown == table_cases.N_CASES  # every case marches something
    print(f"\nnumpy reference vs C restatements, largest colour error: unlit {worst['unlit'][0]:.3g} ({worst['unlit'][1]}), "
          f"lit {worst['lit'][0]:.3g} ({worst['lit'][1]})")


def test_numpy_reference_tile_is_the_frame_cropped(O):
    """The reference's tile (any origin) is the full frame's pixels inside it, zero with zero steps outside."""
    c = next(c for c in table_cases.cases(O) if c.tile is not None)
    cam = O.camera_blob(*c.cam)
    full, fsteps = NR.render(cam, c.vol, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt, light=c.light)
    part, psteps = NR.render(cam, c.vol, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt, light=c.light, tile=c.tile)
    m = tile_mask(c)
    assert (part[m] == full[m]).all() and (psteps[m] == fsteps[m]).all() and fsteps[m].max() > 0
    assert (part[~m] == 0).all() and (psteps[~m] == 0).all()


def tile_mask(c):
    m = np.zeros((c.H, c.W), bool)
    tx, ty, tw, th = c.tile
    m[max(ty, 0):max(ty + th, 0), max(tx, 0):max(tx + tw, 0)] = True
    return m
