"""The histogram kernels (hist_linear_kernel, hist_cells_kernel of vk_launch_hist.hip) on the MI355X over the shared cases
(tests/hist_cases.py), against the C restatement (tests/hist_restatement.c), which the CPU suite holds to an independent numpy reference
(tests/test_hist_fuzz_cpu.py).

For every case and every layout of its format (u8: LINEAR, PACKED, PACKED_PAIRS; f16 and u16: LINEAR, PACKED), through the Python API:
- counts, categories, min and max equal the restatement's BIT FOR BIT, and n_voxels == n_nan + n_below + n_above + sum(counts);
- all layouts of a format are bitwise equal in those;
- sum and sum_sq equal the exact sums for the integer formats and lie within (n - 1) 2^-53 sum|x| of them for f16;
- the same call twice is bitwise equal in everything, the sums included.
A volume is uploaded once per layout and serves all its requests.  The run count and the voxels counted are asserted, so an empty loop
cannot pass.  Every mismatch is collected and reported with the case that shows it."""
import time

import numpy as np
import pytest

import hist_cases
import hist_helpers as HH
import np_hist_reference as NH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return HH.build_restatement(tmp_path_factory.mktemp("hist_fuzz_gpu"))


def _bits64(x):
    return int(np.float64(x).view(np.uint64))


def test_histogram_fuzz_against_the_restatement(V, lib):  # noqa: F811
    start = time.perf_counter()
    cases = hist_cases.cases()
    refs = [(HH.restate_case(lib, c), NH.histogram(c.vol, c.kind, c.bins, c.domain, c.box)) for c in cases]
    fails = []
    runs = voxels = expected_voxels = 0
    first = {}
    by_volume = {}
    for i, c in enumerate(cases):
        by_volume.setdefault(c.vol_id, []).append(i)
    for vol_id, idx in by_volume.items():
        c0 = cases[idx[0]]
        for lay in HH.LAYOUTS[c0.kind]:
            ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)
            try:
                HH.upload(V, ctx, c0.vol, c0.kind, lay)
                for i in idx:
                    c, (ref, exact) = cases[i], refs[i]
                    what = (c.name, lay)
                    got = HH.from_histogram(ctx.volume_histogram(c.bins, c.domain, c.box))
                    again = HH.from_histogram(ctx.volume_histogram(c.bins, c.domain, c.box))
                    runs += 1
                    voxels += got["n_voxels"]
                    expected_voxels += ref["n_voxels"]
                    for msg in HH.integer_part_differences(got, ref):
                        fails.append((what, "against the restatement: " + msg))
                    for msg in HH.sum_differences(got, exact, c.kind):
                        fails.append((what, msg))
                    if HH.integer_part_differences(again, got) or _bits64(again["sum"]) != _bits64(got["sum"]) or _bits64(again["sum_sq"]) != _bits64(got["sum_sq"]):
                        fails.append((what, "the same call twice differs"))
                    if i not in first:
                        first[i] = (lay, got)
                    else:
                        for msg in HH.integer_part_differences(got, first[i][1]):
                            fails.append((what, f"against layout {first[i][0]}: " + msg))
            finally:
                ctx.close()
    elapsed = time.perf_counter() - start
    print(f"\nhistogram fuzz: {len(cases)} cases, {runs} case x layout runs (each twice), {voxels} voxels counted, {elapsed:.1f} s")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    n_u8 = sum(c.kind == "u8" for c in cases)
    assert runs == 3 * n_u8 + 2 * (len(cases) - n_u8) and voxels == expected_voxels and voxels > 1000000
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
