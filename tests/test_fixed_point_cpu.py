"""The cases of tests/fixed_point_cases.py against the C restatements alone: every case really needs the number of rounds or iterations
it is named for, so the list cannot quietly degenerate.  tests/test_fixed_point_gpu.py runs the same cases on the device."""
import numpy as np
import pytest

import fixed_point_cases as FC
import geo_helpers as GH
import skel_helpers as KH
import split_helpers as SH

G_INF = 0xFFFFFFFF


def test_the_batch_constants_and_the_shapes():
    assert (FC.batch("kSplitBatch"), FC.batch("kGeoBatch"), FC.batch("kSkelBatch")) == (8, 8, 4)
    assert FC.counts(8) == (7, 8, 9, 16) and FC.counts(4) == (3, 4, 5, 8)
    for c in [c for _, c in FC.split_cases()] + [c for _, c, _ in FC.geo_cases()] + [c for _, _, c in FC.skel_cases()]:
        assert c.kind == "u8" and c.vol.shape == FC.DIMS[::-1] and c.vol.size <= 70 * 20 * 12
        xs = np.nonzero(c.vol.any(axis=(0, 1)))[0]
        assert xs.min() < 32 <= xs.max(), c.name  # the set spans the tile border at x = 32


def test_split_cases_need_their_rounds(tmp_path):
    lib = SH.build_restatement(tmp_path)
    for rounds, c in FC.split_cases():
        r = SH.restate_case(lib, c)[2]
        assert int(r[7]) == rounds and int(r[2]) == 1 and int(r[5]) == 0 and int(r[1]) == 125 + rounds, (c.name, r)  # one marker; the growth reaches all of S


def test_geodesic_cases_need_their_rounds(tmp_path):
    import vokselis_amd as V

    lib = GH.build_restatement(tmp_path)
    for rounds, c, goal in FC.geo_cases():
        g, _, r = GH.restate_case(lib, c)
        assert int(r[1]) == 1 and int(r[2]) == int(r[0]) == int(c.vol.astype(bool).sum())   # one source; the corridor is reached to its end
        assert int(g[goal[2], goal[1], goal[0]]) == int(r[6]) == 256 * (int(r[0]) - 1)         # ... which is the far end: the path is the corridor
        path = V.geodesic_path(g, goal, c.spacing, c.conn)
        assert len(path) == int(r[0]) and GH.tile_crossings(path) == rounds - 2, (c.name, GH.tile_crossings(path))


def test_skeleton_cases_need_their_iterations(tmp_path):
    lib = KH.build_restatement(tmp_path)
    b = FC.batch("kSkelBatch")
    seen = []
    for needed, budget, c in FC.skel_cases():
        r = KH.restate_case(lib, c)[2]
        it, conv = int(r[KH.R_ITERATIONS]), int(r[KH.R_CONVERGED])
        if budget == 0 or budget > needed:
            assert (it, conv) == (needed, 1), (c.name, it, conv)
        else:
            assert (it, conv) == (budget, 0), (c.name, it, conv)   # every iteration of the budget deleted something: the fixed point was not seen
        seen.append((needed, budget))
    assert seen == [(b - 1, 0), (b, 0), (b + 1, 0), (2 * b, 0), (2 * b, b + 2), (2 * b, b), (2 * b, 2 * b), (2 * b, 5 * b)]
