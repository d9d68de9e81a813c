"""The two references of vk_volume_histogram held together over the shared cases (tests/hist_cases.py): the C
restatement (tests/hist_restatement.c: the rule's operations in order, -ffp-contract=off, fmaf for the one fused operation) and the numpy
reference (tests/np_hist_reference.py: np.float32 operations and a correctly rounded fma of its own, exact sums).

On every case: every count and category equal, min and max bit for bit, n_voxels == n_nan + n_below + n_above + sum(counts).  The
restatement's in-order f64 sums equal the exact ones for the integer formats -- every partial sum is an integer below 2^53 at these sizes --
and lie within the standard bound (n - 1) 2^-53 sum|x| for f16: derived, not measured.  The conditions on the case list -- at least one
voxel of every kind -- are asserted on the restatement's counters, so the list cannot quietly degenerate.

The two exact anchors involve no restatement's arithmetic in their expectation: an R8 volume with 256 bins over [0, 1] has counts ==
bincount(v), an R16_UNORM volume counts == bincount(v >> 8), over all 256 and all 65536 values."""
import numpy as np
import pytest

import hist_cases
import hist_helpers as HH
import np_hist_reference as NH


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return HH.build_restatement(tmp_path_factory.mktemp("hist_fuzz_cpu"))


def test_case_list_covers_the_issue():
    cases = hist_cases.cases()
    assert len({c.name for c in cases}) == len(cases) and 120 <= len(cases) <= 260
    assert {c.kind for c in cases} == {"u8", "f16", "u16"}
    assert {tuple(reversed(c.vol.shape)) for c in cases} == set(hist_cases.DIMS)
    for kind in ("u8", "f16", "u16"):
        mine = [c for c in cases if c.kind == kind]
        assert {c.bins for c in mine} == set(hist_cases.BINS), kind
        assert {c.domain for c in mine} == set(hist_cases.DOMAINS[kind]), kind
        assert any(c.box is None for c in mine) and any(c.box is not None and c.box[0][0] == c.box[1][0] for c in mine), kind
    boxes = [c for c in cases if c.box is not None]
    assert any(all(b - a == 1 for a, b in zip(*c.box)) for c in boxes)                                  # one voxel
    assert any(all(a % 2 == 1 for a in c.box[0]) and all((b - a) % 2 == 1 for a, b in zip(*c.box)) for c in boxes)  # odd origin, odd extent
    for axis in range(3):  # the last plane of an odd dimension alone
        assert any(c.box[0][axis] == c.vol.shape[2 - axis] - 1 and c.vol.shape[2 - axis] % 2 == 1 and c.box[1][axis] == c.vol.shape[2 - axis] for c in boxes), axis
    assert max(c.vol.size for c in cases) <= 24 ** 3


def test_restatement_agrees_with_the_numpy_reference(lib):
    kinds = np.zeros(len(HH.KINDS), np.uint64)
    cases = hist_cases.cases()
    voxels = 0
    worst = 0.0
    for c in cases:
        got = HH.restate_case(lib, c, kinds)
        ref = NH.histogram(c.vol, c.kind, c.bins, c.domain, c.box)
        assert not HH.integer_part_differences(got, ref), (c.name, HH.integer_part_differences(got, ref))
        assert not HH.sum_differences(got, ref, c.kind), (c.name, HH.sum_differences(got, ref, c.kind))
        if c.kind == "f16" and ref["n_finite"] > 1 and ref["abs_sum"] > 0:
            worst = max(worst, float(NH.sum_error(got["sum"], ref["sum"]) / NH.sum_bound(ref["n_finite"], ref["abs_sum"])))
        lo, hi = hist_cases.box_of(c)
        assert got["n_voxels"] == (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
        voxels += got["n_voxels"]
        if "all NaN" in c.name and got["n_voxels"]:
            assert got["n_nan"] == got["n_voxels"] and got["min"] == np.inf and got["max"] == -np.inf and got["n_finite"] == 0
        if got["n_voxels"] == 0:
            assert got["min"] == np.inf and got["max"] == -np.inf and got["sum"] == 0.0 and not got["counts"].any()
    print(f"\nhistogram cases: {len(cases)} cases, {voxels} voxels; voxels of each kind on the restatement: "
          + ", ".join(f"{k} {int(v)}" for k, v in zip(HH.KINDS, kinds)) + f"; the f16 sums use at most {worst:.3g} of their bound")
    for k, v in zip(HH.KINDS, kinds):
        assert v > 0, k


def test_min_and_max_order_negative_zero_below_positive_zero(lib):
    vol = np.array([[[0.0, -0.0, 0.0, -0.0, 0.0]]], np.float16)
    for got in (HH.restate(lib, vol, "f16", 4, (0.0, 1.0)), NH.histogram(vol, "f16", 4, (0.0, 1.0))):
        assert HH.bits(got["min"]) == 0x80000000 and HH.bits(got["max"]) == 0 and int(got["counts"][0]) == 5


def all_values(kind):
    if kind == "u8":
        return np.arange(256, dtype=np.uint8).reshape(4, 8, 8)
    return np.random.default_rng(5).permutation(65536).astype(np.uint16).reshape(16, 64, 64)


@pytest.mark.parametrize("kind, shift", [("u8", 0), ("u16", 8)])
def test_exact_anchor_over_every_value(lib, kind, shift):
    vol = all_values(kind)
    want = np.bincount((vol.ravel().astype(np.int64) >> shift), minlength=256).astype(np.uint64)
    for got in (NH.histogram(vol, kind, 256, (0.0, 1.0)), HH.restate(lib, vol, kind, 256, (0.0, 1.0))):
        assert (got["counts"] == want).all() and got["n_below"] == got["n_above"] == got["n_nan"] == 0
    # ... and on a box of it
    box = ((1, 2, 1), (8, 7, 4)) if kind == "u8" else ((3, 5, 2), (64, 61, 15))
    sub = vol[box[0][2]:box[1][2], box[0][1]:box[1][1], box[0][0]:box[1][0]]
    want = np.bincount((sub.ravel().astype(np.int64) >> shift), minlength=256).astype(np.uint64)
    for got in (NH.histogram(vol, kind, 256, (0.0, 1.0), box), HH.restate(lib, vol, kind, 256, (0.0, 1.0), box)):
        assert (got["counts"] == want).all()
