"""The built-in transfer function of VK_MODE_NAIVE_TRILINEAR (no table) on the CPU, over the shared fuzz cases (tests/builtin_cases.py):
the C oracle held to an independent numpy reference (tests/np_builtin_reference.py: the alpha chain in f32, the palette, compositing and
linear_to_srgb in float64), and the skip maps' emptiness predicate (vk_tf.hpp: builtin_cell_empty) held to transfer_alpha -- sample by
sample on every case, and by a host fuzz under ASan + UBSan (tests/builtin_fuzz.cpp) over every f16 pattern and random edge cells."""
import os
import subprocess

import numpy as np
import pytest

import builtin_cases
import np_builtin_reference as NB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("builtin_fuzz") / "builtin_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "builtin_fuzz.cpp")], check=True)
    return exe


def rel_err(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.maximum(1.0, np.abs(ref.astype(np.float64)))


def test_case_list_covers_the_edges(O):
    """The list is the one the GPU fuzz walks; what it must hold does not depend on the draw."""
    cases = builtin_cases.cases(O)
    assert len(cases) == builtin_cases.N_CASES == 58
    assert {c.dt for c in cases} == set(builtin_cases.DTS)
    assert {c.kind for c in cases} == {0, 1, 2, 3}
    for f16 in (False, True):
        assert {c.dt for c in cases if c.f16 == f16} == set(builtin_cases.DTS), f16
        assert {c.kind for c in cases if c.f16 == f16} == {0, 1, 2, 3}, f16
    bits = np.concatenate([c.vol.view(np.uint16).ravel() for c in cases if c.f16])
    for name, b in builtin_cases.F16_EDGE_BITS.items():
        assert (bits == b).any(), name
    u8 = np.concatenate([c.vol.ravel() for c in cases if not c.f16])
    for v in builtin_cases.U8_EDGES:
        assert (u8 == v).any(), v
    names = {c.name: c for c in cases}
    for name, empty in (("-inf ball in air", None), ("-inf throughout", 0.0), ("NaN ball in air", None), ("+inf ball in air", None),
                        ("air of -0, subnormals and negatives", 1.0), ("all 25", 1.0), ("all 26", 0.0)):
        assert names[name].empty == empty, name
    assert {names[n].f16 for n in ("-inf ball in air", "NaN ball in air", "+inf ball in air", "-inf throughout")} == {True}
    assert (names["-inf throughout"].vol.view(np.uint16) == 0xFC00).all()
    assert NB.cell_empty([names["air of -0, subnormals and negatives"].vol.astype(np.float32)], True).all()
    assert set(np.unique(names["0/255 checkerboard"].vol)) == {0, 255}
    assert {25, 26} <= set(np.unique(names["25 air, lone 26 speckles"].vol)) and {254, 255} & set(np.unique(names["254/255 blocks"].vol))
    for dims in builtin_cases.FIXED_DIMS:
        assert any(c.dims == dims for c in cases), dims
    rdims = [d for c in cases if "random dims" in c.tags for d in c.dims]
    assert min(rdims) >= 3 and max(rdims) <= 72 and max(rdims) >= 60
    assert any(d % 4 in (1, 3) for d in rdims) and any(d % 8 in (1, 7) for d in rdims) and any(d % 8 == 0 for d in rdims)
    assert {c.W % 2 for c in cases} == {0, 1} and {c.H % 2 for c in cases} == {0, 1}
    assert min(min(c.W, c.H) for c in cases) >= 24 and max(max(c.W, c.H) for c in cases) <= 96
    assert sum(c.tile is not None for c in cases) >= 3 and any(c.tile is not None and min(c.tile[:2]) < 0 for c in cases)
    assert any(c.half and c.f16 for c in cases) and any(c.half and not c.f16 for c in cases)
    assert sum(c.edge for c in cases) >= 20


def test_numpy_reference_agrees_with_the_oracle(O):
    """Equal step counts, equal sampled counts (the oracle's emptiness and the reference's own), colour within 2e-5 relative to max(1, |ref|),
    everything finite: the built-in colour is vertigo(alpha), finite even for NaN data."""
    worst = (0.0, None)
    for c in builtin_cases.cases(O):
        cam = O.camera_blob(*c.cam)
        ref, ref_steps, ref_sampled = O.render(cam, c.vol, c.W, c.H, dt_scale=c.dt, tile=c.tile)
        got, steps, sampled = NB.render(cam, c.vol, c.W, c.H, dt=c.dt, tile=c.tile)
        assert (steps == ref_steps).all(), (c, int((steps != ref_steps).sum()))
        assert (sampled == ref_sampled).all(), (c, int((sampled != ref_sampled).sum()))
        assert np.isfinite(ref).all() and np.isfinite(got).all(), c
        err = float(rel_err(got, ref[..., :3]).max())
        assert err <= TOL, (c, err)
        if err >= worst[0]:
            worst = (err, c.name)
        assert ref_steps.max() > 0, c  # every case marches something
    print(f"\nnumpy reference vs the C oracle, largest colour error: {worst[0]:.3g} ({worst[1]})")


def test_empty_cells_sample_zero_alpha(O, fuzz_exe):
    """The skip maps' promise: every sample the reference takes in a cell that the predicate calls empty has alpha exactly +0.  The numpy
    predicate is first held to the library's (vk_tf.hpp, through the fuzz binary) on every f16 pattern and every u8 value."""
    r = subprocess.run([fuzz_exe, "taps"], capture_output=True, text=True, timeout=120, check=True)
    lib_f16, lib_u8 = (np.frombuffer(line.encode(), np.uint8) == ord("1") for line in r.stdout.split())
    assert lib_f16.size == 65536 and lib_u8.size == 256
    assert (NB.tap_empty(np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32), True) == lib_f16).all()
    assert (NB.tap_empty(np.arange(256, dtype=np.float32), False) == lib_u8).all()
    total = {"empty": 0, "bad": 0}
    bad_cases = []
    for c in builtin_cases.cases(O):
        seen = {"empty": 0, "bad": 0}

        def on_sample(a, empty):
            seen["empty"] += int(empty.sum())
            seen["bad"] += int(((a != 0) | np.signbit(a))[empty].sum())

        NB.render(O.camera_blob(*c.cam), c.vol, c.W, c.H, dt=c.dt, tile=c.tile, on_sample=on_sample)
        if seen["bad"]:
            bad_cases.append((c.name, seen["bad"]))
        for k in total:
            total[k] += seen[k]
    assert not bad_cases, f"samples with alpha != +0 in cells called empty: {bad_cases}"
    assert total["empty"] > 100000, total  # (the cases reach empty cells)


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15"])
def test_builtin_predicate_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "100000", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    bad, empty = r.stdout.split("bad ")[1].split(" of ")[0], r.stdout.split("(")[-1].split(" empty")[0]
    assert bad == "0" and int(empty) > 1000, r.stdout  # (the fuzz must actually reach empty cells)
