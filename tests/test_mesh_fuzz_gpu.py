"""The mesh kernels (mesh_count_kernel, mesh_scan_kernel, mesh_emit_kernel of vk_launch_mesh.hip) on the MI355X over the shared cases
(tests/mesh_cases.py), against the C restatement (tests/mesh_restatement.c), which the CPU suite holds to an independent numpy reference
(tests/test_mesh_fuzz_cpu.py).

For every case and every layout of its format (u8: LINEAR, PACKED, PACKED_PAIRS; f16 and u16: LINEAR, PACKED), through the Python API:
- the count and the triangles equal the restatement's BIT FOR BIT;
- all layouts of a format are therefore bitwise equal, which is asserted too;
- the same call twice is bitwise equal.
A volume is uploaded once per layout and serves all its boxes.  The run count and the triangles compared are asserted, so an empty loop
cannot pass.  Every mismatch is collected and reported with the case that shows it."""
import time

import pytest

import mesh_cases
import mesh_helpers as MH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return MH.build_restatement(tmp_path_factory.mktemp("mesh_fuzz_gpu"))


def test_mesh_fuzz_against_the_restatement(V, lib):  # noqa: F811
    start = time.perf_counter()
    cases = mesh_cases.cases()
    refs = [MH.restate_case(lib, c) for c in cases]
    fails = []
    runs = triangles = expected = 0
    first = {}
    by_volume = {}
    for i, c in enumerate(cases):
        by_volume.setdefault(c.vol_id, []).append(i)
    for vol_id, idx in by_volume.items():
        c0 = cases[idx[0]]
        for lay in MH.LAYOUTS[c0.kind]:
            ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)
            try:
                MH.upload(V, ctx, c0.vol, c0.kind, lay)
                for i in idx:
                    c, ref = cases[i], refs[i]
                    what = (c.name, lay)
                    got = ctx.extract_isosurface(c.iso, c.box)
                    again = ctx.extract_isosurface(c.iso, c.box)
                    runs += 1
                    triangles += len(got)
                    expected += len(ref)
                    if len(got) != len(ref):
                        fails.append((what, f"{len(got)} triangles, the restatement has {len(ref)}"))
                    elif not MH.same_bits(got, ref):
                        bad = (got.view("u4") != ref.view("u4")).any(axis=(1, 2)).nonzero()[0]
                        fails.append((what, f"{len(bad)} of {len(ref)} triangles differ from the restatement, the first at {int(bad[0])}: {got[bad[0]].tolist()} != {ref[bad[0]].tolist()}"))
                    if not MH.same_bits(again, got):
                        fails.append((what, "the same call twice differs"))
                    if i not in first:
                        first[i] = (lay, got)
                    elif not MH.same_bits(got, first[i][1]):
                        fails.append((what, f"differs from layout {first[i][0]}"))
            finally:
                ctx.close()
    elapsed = time.perf_counter() - start
    print(f"\nmesh fuzz: {len(cases)} cases, {runs} case x layout runs (each twice), {triangles} triangles compared, {elapsed:.1f} s")
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    n_u8 = sum(c.kind == "u8" for c in cases)
    assert runs == 3 * n_u8 + 2 * (len(cases) - n_u8) and triangles == expected and triangles > 1000000
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
