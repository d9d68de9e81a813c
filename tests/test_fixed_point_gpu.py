"""The batched fixed-point loop of the split, geodesic and skeleton passes (PassCall::iterate) at its batch
boundaries, on the MI355X: the cases of tests/fixed_point_cases.py -- B - 1, B, B + 1 and 2 B rounds, and the skeleton's budget inside a
batch, on a batch's last iteration and beyond convergence -- with every array, every total and rounds / iterations / converged bitwise
equal to the C restatements, and the launch counts the loop's rules give: whole batches, cut short by the budget alone.  No tolerance.
The geodesic launches are B ceil(rounds / B): the last round that visits a tile is also the one that wakes none, so the batch that holds
it is the last (the loop before PassCall::iterate gave the same counts on these cases: 8, 8, 16 and 16 launches for 7, 8, 9 and 16 rounds)."""
import numpy as np
import pytest

import fixed_point_cases as FC
import geo_helpers as GH
import label_helpers as LH
import skel_helpers as KH
import split_helpers as SH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx(V):  # noqa: F811
    c = V.Context(64, 64, V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), 1.0), backbuffer=(64, 64), out_format=V.OUT_RGBA32F)
    yield c
    c.close()


def _message(V, ctx):  # noqa: F811
    """The totals a pass leaves as the context's last message under X_timing 9: {name: value}."""
    words = V.native.lib().vk_last_error(ctx.handle).decode().split()
    return {words[k]: int(words[k + 1]) for k in range(1, len(words) - 1, 2)}


def _whole_batches(rounds, b):
    return b * -(-rounds // b)


def test_split_growth_at_the_batch_boundaries(V, ctx, tmp_path):  # noqa: F811
    lib = SH.build_restatement(tmp_path)
    for rounds, c in FC.split_cases():
        labels, table, result, dense, _ = SH.restate_case(lib, c)
        LH.upload(V, ctx, c.vol, "u8", "LINEAR")
        rc, got = SH.run(V, ctx, c)
        assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
        assert int(got[2][7]) == rounds == int(result[7]), (c.name, got[2])
        assert LH.differences(got, (labels, table, result, dense)) == "", c.name


def test_geodesic_rounds_at_the_batch_boundaries(V, ctx, tmp_path):  # noqa: F811
    lib = GH.build_restatement(tmp_path)
    b = FC.batch("kGeoBatch")
    ctx.set_param("geo_timing", 9)
    for rounds, c, _ in FC.geo_cases():
        want = GH.restate_case(lib, c)
        LH.upload(V, ctx, c.vol, "u8", "LINEAR")
        rc, got = GH.run(V, ctx, c)
        assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
        m = _message(V, ctx)
        print(c.name, m)
        assert GH.differences(got, want) == "", c.name
        # the corridor's crossings + 2 rounds visit a tile, and the last of them is the one that wakes nothing (fixed_point_cases.py):
        # the batch that holds it is the last, and it is launched whole
        assert m["rounds"] == rounds and m["launches"] == _whole_batches(rounds, b), (c.name, m)


def test_skeleton_iterations_and_budget_at_the_batch_boundaries(V, ctx, tmp_path):  # noqa: F811
    lib = KH.build_restatement(tmp_path)
    b = FC.batch("kSkelBatch")
    ctx.set_param("skel_timing", 9)
    for needed, budget, c in FC.skel_cases():
        want = KH.restate_case(lib, c)
        LH.upload(V, ctx, c.vol, "u8", "LINEAR")
        rc, got = KH.run(V, ctx, c)
        assert rc == 0, (c.name, V.native.lib().vk_last_error(ctx.handle))
        m = _message(V, ctx)
        print(c.name, m)
        assert KH.differences(got, want) == "", c.name
        stopped = budget != 0 and budget <= needed
        assert (int(got[2][KH.R_ITERATIONS]), int(got[2][KH.R_CONVERGED])) == ((budget, 0) if stopped else (needed, 1)), (c.name, got[2])
        # iteration needed + 1 is the one that deletes nothing: whole batches up to the one that holds it, no iteration beyond the budget;
        # eight sub-pass launches an iteration
        enqueued = _whole_batches(needed + 1, b)
        assert m["iterations"] == (budget if stopped else needed) and m["launches"] == 8 * (min(enqueued, budget) if budget else enqueued), (c.name, m)
