"""The compute twin (VK_MODE_COMPUTE_NEAREST) on the CPU, over the shared fuzz cases (tests/compute_cases.py): the C oracle held to an
independent numpy reference (tests/np_compute_reference.py: t, p and the alpha chain in f32, shading and compositing in float64), and the
records' emptiness predicate (vk_pair.hpp: pair_record_empty) held to the records kernel's step arithmetic by a host fuzz under
ASan + UBSan (tests/compute_fuzz.cpp) over every f16 opacity pattern crossed with colour and normal edge patterns."""
import os
import subprocess

import numpy as np
import pytest

import compute_cases
import np_compute_reference as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("compute_fuzz") / "compute_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "compute_fuzz.cpp")], check=True)
    return exe


def colour_mismatch(got, ref, tol):
    """(largest error over the finite pixels, count of pixels whose non-finite values differ).  Finite: |got - ref| / max(1, |ref|);
    non-finite: NaN exactly where the reference has NaN, an infinity exactly where it has the same one."""
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    fin = np.isfinite(ref) & np.isfinite(got)
    err = float((np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))).max(initial=0.0))
    odd = ~fin & ~((np.isnan(got) & np.isnan(ref)) | (got == ref))
    return err, int(odd.any(axis=-1).sum())


def test_case_list_covers_the_edges(O):
    """The list is the one the GPU fuzz walks; what it must hold does not depend on the draw."""
    cases = compute_cases.cases(O)
    assert len(cases) == compute_cases.N_CASES == 62
    assert set(compute_cases.DTS) <= {c.dt for c in cases if "random dims" in c.tags}
    assert {c.kind for c in cases} == {0, 1, 2, 3, 4}
    assert max(c.dt for c in cases) == 3.5 and min(c.dt for c in cases) < 0.0135
    for where, get in (("colour", lambda c: c.den.view(np.uint16)[..., :3]), ("opacity", lambda c: c.den.view(np.uint16)[..., 3]),
                       *((f"normal {k}", lambda c, k=k: c.nrm.view(np.uint16)[..., k]) for k in range(3))):
        bits = np.concatenate([get(c).ravel() for c in cases if c.edge])
        for name, b in compute_cases.F16_EDGE_BITS.items():
            assert (bits == b).any(), (where, name)
    op = np.concatenate([c.den.view(np.uint16)[..., 3].ravel() for c in cases])
    for b in compute_cases.TINY_OPACITY_BITS + compute_cases.ZERO_OPACITY_BITS:
        assert (op == b).any(), hex(b)
    assert sum(c.divergent for c in cases) <= 6 and any(c.divergent for c in cases)
    assert all(not c.divergent for c in cases if "non-finite air" in c.tags)
    assert sum("non-finite air" in c.tags for c in cases) >= 8 and sum("xor" in c.tags for c in cases) >= 5
    dims = [d for c in cases for d in c.dims]
    assert min(dims) == 1 and any(d % 4 in (1, 3) for d in dims) and max(d for c in cases if "walk" not in c.tags for d in c.dims) <= 72
    assert sum("walk" in c.tags and max(c.dims) >= 128 for c in cases) >= 5 and max(dims) == 256
    far = [c for c in cases if c.kind == 4]
    assert len(far) >= 8 and min(c.cam[0] for c in far) >= 10 and any(c.cam[0] > 100 for c in far)
    assert sum(10 <= c.cam[0] <= 60 for c in far) >= 7
    assert sum(c.tile is not None for c in cases) >= 12 and any(c.tile is not None and min(c.tile[:2]) < 0 for c in cases)
    assert any(c.tile is not None and c.tile[0] >= c.W for c in cases)
    assert sum(c.half for c in cases) >= 6
    assert len(compute_cases.procedural_cases()) == 10 and max(p[7] for p in compute_cases.procedural_cases()) >= 1e5


def test_far_eyes_see_the_box(O):
    """A far eye (10..60 units) still puts at least 20 x 20 pixels of the box in its tile."""
    for c in compute_cases.cases(O):
        if c.kind != 4 or c.cam[0] > 60:
            continue
        _, steps, _ = O.render(O.camera_blob(*c.cam), c.den, c.W, c.H, mode=O.MODE_COMPUTE_NEAREST, volume2=c.nrm, dt_scale=max(c.dt, 1.0),
                               tile=c.tile)
        ys, xs = np.nonzero(steps)
        assert xs.size and xs.max() - xs.min() + 1 >= 20 and ys.max() - ys.min() + 1 >= 20, c


def test_walk_cases_run_down_their_long_axis(O, R):
    """Every walk case's rays (at the corners and the centre of the pixels the CPU checks) cross its long axis: the largest direction
    component, in voxels, is on it, and the ray crosses at least 100 voxels of it in the box.  At the far eyes that drift, the 0.01 floor
    binds (dt = 0.01 dt_scale), dt / ulp(t0) is the DRIFT_ULPS the cases are built on, and t0 + dt rounds up."""
    walks = [c for c in compute_cases.cases(O) if "walk" in c.tags]
    assert len(walks) == 8 and sum("slab" in c.tags for c in walks) == 2
    for c in walks:
        long = int(np.argmax(c.dims))
        ray = R.compute_rays(O.camera_blob(*c.cam), c.dims, c.W, c.H, c.dt, c.crop)
        d = np.abs(np.stack(ray["d"]).astype(np.float64)) * np.array(c.dims, np.float64)[:, None]
        assert ray["hit"].all() and (np.argmax(d, axis=0) == long).all(), (c, d)
        cross = (ray["t1"] - ray["t0"]).astype(np.float64) * np.abs(ray["d"][long]) * c.dims[long] / 2
        assert (cross >= 100).all(), (c, cross)
        if "far" in c.tags:
            dtv = 1.0 / (np.array(c.dims, np.float32)[:, None] * np.abs(np.stack(ray["d"])))
            assert (dtv.min(axis=0) < 0.01).all() and (ray["dt"] == np.float32(c.dt * np.float32(0.01))).all(), c
            t0, dt = ray["t0"], ray["dt"]
            ulp = np.spacing(t0)
            assert np.allclose(dt / ulp, compute_cases.DRIFT_ULPS[c.name], atol=0.01), (c, dt / ulp)
            assert ((t0 + dt).astype(np.float32) - t0 > dt).all(), c


def test_numpy_reference_agrees_with_the_oracle(O):
    """Equal step counts; colour within 2e-5 relative to max(1, |ref|); NaN and infinities exactly where the oracle has them.  The long
    rays of the walk cases are checked on a few pixels (`crop`)."""
    worst = (0.0, None)
    nonfinite = 0
    for c in compute_cases.cases(O):
        cam = O.camera_blob(*c.cam)
        tile = c.crop or c.tile
        ref, ref_steps, _ = O.render(cam, c.den, c.W, c.H, mode=O.MODE_COMPUTE_NEAREST, volume2=c.nrm, dt_scale=c.dt, tile=tile)
        got, steps = NC.render(cam, c.den, c.nrm, c.W, c.H, dt=c.dt, tile=tile)
        assert (steps == ref_steps).all(), (c, int((steps != ref_steps).sum()))
        err, odd = colour_mismatch(got, ref[..., :3], TOL)
        assert err <= TOL and odd == 0, (c, err, odd)
        if err >= worst[0]:
            worst = (err, c.name)
        nonfinite += int((~np.isfinite(ref[..., :3])).any(axis=-1).sum())
        assert ref_steps.max() > 0 or c.tile == (64, 0, 32, 32), c  # every case marches something (but the tile off screen)
    assert nonfinite > 100  # (the edge cases reach NaN and infinite colours)
    print(f"\nnumpy reference vs the C oracle, largest colour error: {worst[0]:.3g} ({worst[1]}); {nonfinite} non-finite pixels")


def test_opacity_term_matches_the_library(fuzz_exe):
    """The reference's f32 opacity term is zero on exactly the f16 patterns where the library's (vk_pair.hpp) is."""
    r = subprocess.run([fuzz_exe, "opacity"], capture_output=True, text=True, timeout=120, check=True)
    lib = np.frombuffer(r.stdout.strip().encode(), np.uint8) == ord("1")
    assert lib.size == 65536
    ref = NC.opacity(np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)) == 0
    assert (ref == lib).all(), np.nonzero(ref != lib)[0][:10]
    assert lib[0x8000:].all() and lib[0] and not lib[1:0x7C00].any()  # (<= 0 and NaN: zero; every positive f16, subnormals too: not)


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15"])
def test_record_predicate_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "200000", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    out = r.stdout.split("bad ")[1]
    bad, empty, kept = out.split(" of ")[0], out.split("(")[1].split(" empty")[0], out.split(", ")[1].split(" kept")[0]
    # (the fuzz must reach empty records, and records whose zero opacity term does not make them empty)
    assert bad == "0" and int(empty) > 100000 and int(kept) > 10000, r.stdout
