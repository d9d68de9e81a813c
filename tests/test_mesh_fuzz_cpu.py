"""The two references of vk_extract_isosurface held together over the shared cases (tests/mesh_cases.py): the C
restatement (tests/mesh_restatement.c: the rule's operations in order, -ffp-contract=off) and the numpy reference
(tests/np_mesh_reference.py: whole-array np.float32 operations, sorted into the stated order) -- triangle for triangle, bit for bit.  The
conditions on the case list -- at least one cube of every kind -- are asserted on the restatement's counters, so the list cannot quietly
degenerate.

The properties of the rule are asserted on the restatement's output: the 256 corner configurations of a cube, closedness, orientation,
Euler characteristic and volume of a ball and a torus, and the direction of every triangle's normal.  The manifold cases use a threshold at
a half-integer on integer data, so no vertex lands on a lattice point and welding by bit pattern is exact."""
import numpy as np
import pytest

import mesh_cases
import mesh_helpers as MH
import np_mesh_reference as NM


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return MH.build_restatement(tmp_path_factory.mktemp("mesh_fuzz_cpu"))


def test_case_list_covers_the_issue():
    cases = mesh_cases.cases()
    assert len({c.name for c in cases}) == len(cases) and 100 <= len(cases) <= 260
    assert {tuple(reversed(c.vol.shape)) for c in cases} == set(mesh_cases.DIMS)
    for kind in ("u8", "f16", "u16"):
        names = " | ".join(c.name for c in cases if c.kind == kind)
        for word in ("constant", "two-valued", "uniform", "ball", "whole", "empty", "one voxel thick", "odd origin", "low faces", "high faces"):
            assert word in names, (kind, word)
    assert any("torus" in c.name for c in cases) and any("NaN, inf" in c.name and c.kind == "f16" for c in cases)
    assert max(c.vol.size for c in cases) <= 24 ** 3


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(lib):
    kinds = np.zeros(MH.N_KINDS, np.uint64)
    total = 0
    for c in mesh_cases.cases():
        got = MH.restate_case(lib, c, kinds)
        ref = NM.mesh(c.vol, c.kind, c.iso, c.box)
        assert MH.same_bits(got, ref), (c.name, got.shape, ref.shape)
        if c.box is not None and any(b - a < 2 for a, b in zip(*c.box)):
            assert len(got) == 0, c.name
        if "constant" in c.name:
            assert len(got) == 0, c.name
        total += len(got)
    per_tet = kinds[4:].reshape(6, 16)
    print(f"\nmesh cases: {len(mesh_cases.cases())} cases, {total} triangles; cubes skipped for a non-finite corner {int(kinds[0])}, all inside {int(kinds[1])}, "
          f"vertices with f == 0 {int(kinds[2])}, f == 1 {int(kinds[3])}; fewest tetrahedra of a (k, mask) pair {int(per_tet[:, 1:15].min())}")
    assert total > 100000
    assert kinds[0] > 0 and kinds[1] > 0 and kinds[2] > 0 and kinds[3] > 0
    assert (per_tet[:, 1:15] > 0).all(), per_tet


def _all_configurations():
    for cfg in range(256):
        yield cfg, (np.array([(cfg >> b) & 1 for b in range(8)], np.uint8) * 255).reshape(2, 2, 2)


def test_the_256_corner_configurations(lib):
    total = 0
    for cfg, cube in _all_configurations():
        alone = MH.restate_k(lib, cube, "u8", 127.5)
        assert len(alone) <= 12, cfg
        total += len(alone)
        vol = np.zeros((4, 4, 4), np.uint8)
        vol[1:3, 1:3, 1:3] = cube
        tris = MH.restate_k(lib, vol, "u8", 127.5)
        if cfg == 0:
            assert len(tris) == 0
            continue
        verts, faces = MH.weld(tris)
        assert MH.edge_report(faces) == (True, True), cfg
        assert MH.signed_volume(tris) > 0.0, cfg
    assert total == 1920


def test_ball_is_a_closed_oriented_sphere_of_the_right_volume(lib):
    n = 24
    vol = mesh_cases.ball((n, n, n), "u8")
    assert not vol[0].any() and not vol[:, 0].any() and not vol[:, :, 0].any() and not vol[-1].any() and not vol[:, -1].any() and not vol[:, :, -1].any()
    tris = MH.restate_k(lib, vol, "u8", 127.5)
    verts, faces = MH.weld(tris)
    assert MH.edge_report(faces) == (True, True) and MH.euler(verts, faces) == 2
    vol_mesh = MH.signed_volume(tris)
    # The field is g(p) = 1.3 - 3.2 |p - c| in unit-cube coordinates, the threshold g = 0.5 at |p - c| = R = 0.25.  The mesh is the level set
    # of the piecewise-linear interpolant of the stored field over tetrahedra of diameter h = sqrt(3) / n.  Linear interpolation errs by at
    # most h^2 / 2 times the largest second derivative, which for 3.2 |p - c| is 3.2 / |p - c| <= 3.2 / (R - 2 h) in the cells the surface
    # can reach; rounding to u8 adds 0.5 / 255, and the threshold 127.5 / 255 is 0.5 exactly.  So the surface lies where |g - 0.5| <= eps,
    # i.e. within delta = eps / 3.2 of the sphere, and the enclosed volume between the balls of radius R -+ delta.
    h, R = np.sqrt(3.0) / n, 0.25
    eps = 0.5 * h * h * 3.2 / (R - 2.0 * h) + 0.5 / 255.0
    delta = eps / 3.2
    lo, hi = 4.0 / 3.0 * np.pi * (R - delta) ** 3, 4.0 / 3.0 * np.pi * (R + delta) ** 3
    print(f"\nball: {len(tris)} triangles, volume {vol_mesh:.5f}, analytic {4.0 / 3.0 * np.pi * R ** 3:.5f}, allowed [{lo:.5f}, {hi:.5f}]")
    assert vol_mesh > 0.0 and lo <= vol_mesh <= hi


def test_torus_has_euler_characteristic_zero(lib):
    vol = mesh_cases.torus((24, 24, 24), "u8")
    tris = MH.restate_k(lib, vol, "u8", 127.5)
    verts, faces = MH.weld(tris)
    assert len(tris) > 1000 and MH.edge_report(faces) == (True, True) and MH.euler(verts, faces) == 0
    assert MH.signed_volume(tris) > 0.0


def test_random_volume_in_a_zero_border_welds_into_a_closed_oriented_surface(lib):
    vol = np.zeros((10, 11, 12), np.uint8)
    vol[1:-1, 1:-1, 1:-1] = np.random.default_rng(4).integers(0, 256, (8, 9, 10))
    tris = MH.restate_k(lib, vol, "u8", 127.5)
    verts, faces = MH.weld(tris)
    assert len(tris) > 1000 and MH.edge_report(faces) == (True, True)


@pytest.mark.parametrize("which", ["ball", "torus", "random"])
def test_normals_point_from_the_inside_corners_to_the_outside_corners(lib, which):
    """The tetrahedron of a triangle is recovered from its centroid: the cube from the integer part of centroid * n - 0.5, the permutation
    from the order of the fractional parts (v1 = v0 + e[the axis of the largest], ...).  In it the field is linear, so the direction from
    the mean of its inside vertices to the mean of its outside vertices has a negative slope, and the normal -- towards lower values -- a
    non-negative dot product with it."""
    n = 24
    vol = {"ball": mesh_cases.ball((n, n, n), "u8"), "torus": mesh_cases.torus((n, n, n), "u8"),
           "random": np.random.default_rng(6).integers(0, 256, (n, n, n)).astype(np.uint8)}[which]
    tris = MH.restate_k(lib, vol, "u8", 127.5)
    nrm = MH.normals(tris)
    cen = tris.astype(np.float64).mean(axis=1) * n - 0.5
    low = np.floor(cen).astype(int)
    frac = cen - low
    order = np.argsort(-frac, axis=1, kind="stable")  # the axes by decreasing fractional part
    eye = np.eye(3, dtype=int)
    tv = [np.zeros_like(low), eye[order[:, 0]], eye[order[:, 0]] + eye[order[:, 1]], np.ones_like(low)]
    inside_sum, outside_sum = np.zeros((len(tris), 3)), np.zeros((len(tris), 3))
    n_in = np.zeros(len(tris))
    for v in tv:
        p = low + v
        val = vol[p[:, 2], p[:, 1], p[:, 0]].astype(np.float64)
        ins = val >= 127.5
        inside_sum += np.where(ins[:, None], v, 0)
        outside_sum += np.where(ins[:, None], 0, v)
        n_in += ins
    assert ((n_in >= 1) & (n_in <= 3)).all()
    d = outside_sum / (4 - n_in)[:, None] - inside_sum / n_in[:, None]
    dots = np.einsum("ij,ij->i", nrm * n * n, d)
    assert len(tris) > 1000 and (dots >= 0.0).all(), float(dots.min())
    assert (dots > 0.0).mean() > 0.99
