"""The rule that sends a cell march down its unclamped build (vk_hostmath.hpp: cell_march_fast), audited on the CPU.

tests/fastpath_fuzz.cpp, built with AddressSanitizer and UBSan and linked with tests/shadow_restatement.c and the oracle, replays rays
with the restatement's own f32 loops and asserts that wherever the rule says "fast" every looked-up index lies inside the index tables;
it holds the tables' entries and the clamped march's offsets to the 64-bit closed form on every kind of shape the upload accepts; and it
checks itself: on seven fixed rows a rule that looks at the camera's distance alone, kept in the program, must be seen to overrun.

The rest is about the cases the GPU module runs (tests/fastpath_cases.py), decided here by the references alone: the list's conditions,
this module's statement of the rule against the header's, the replay audit of every case the rule calls fast, the C references against
the numpy references on the cases short enough for numpy, and that the configurations bench.py times keep the unclamped build."""
import dataclasses
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import fastpath_cases as FC
import np_builtin_reference as NB
import np_table_reference as NR
import np_u16_reference as NU
import tf_helpers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
TOL = 2e-5  # the numpy references against the C references (test_builtin_fuzz_cpu.py, test_table_fuzz_cpu.py)


@pytest.fixture(scope="module")
def fuzz_exe(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("fastpath")
    so_oracle = O.build()
    obj, exe = str(d / "shadow_restatement.o"), str(d / "fastpath_fuzz")
    subprocess.run(["gcc", "-O1", "-g", "-ffp-contract=off", *SAN, "-I", os.path.join(ROOT, "oracle"), "-c", "-o", obj,
                    os.path.join(ROOT, "tests", "shadow_restatement.c")], check=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *SAN, "-I", os.path.join(ROOT, "vokselis_amd", "csrc"),
                    "-I", os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(ROOT, "tests", "fastpath_fuzz.cpp"), obj, so_oracle,
                    "-Wl,-rpath," + os.path.dirname(so_oracle), "-lm"], check=True)
    return exe


def _run(exe, *args, timeout=600):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout, env=ENV)
    assert r.returncode == 0, (args, r.stdout[-3000:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261021"])
def test_fastpath_audit_under_sanitizers(fuzz_exe, seed):
    out = _run(fuzz_exe, 600, seed)
    assert out.strip().endswith("OK (600 cases)"), out[-3000:]
    # the self-check ran: the distance-only rule is seen to overrun on each of the seven rows, to at least the index fastpath_cases.ROWS records
    rows = re.findall(r"row (\d+) x 4 x 4, camera ([\d.]+) away, dt ([\d.]+): longest ray (\d+) trips, x index up to (\d+) .*distance-only rule fast, the rule safe", out)
    assert len(rows) == len(FC.ROWS) == 7, out[-3000:]
    for (nx, dist, dt, seen), row in zip(FC.ROWS, rows):
        assert (int(row[0]), float(row[1]), float(row[2])) == (nx, dist, dt) and int(row[4]) >= seen > nx, (row, seen)
    assert re.search(r"offsets: \d+ accepted shapes, \d+ arrays of 4 GiB and more", out)


def _header_rule(exe, dims, eye, dt, flags=0, cell_bytes=8):
    return _run(exe, "rule", *dims, *(repr(float(e)) for e in eye), repr(float(dt)), flags, cell_bytes).strip() == "fast"


def _audit(exe, O, c, tmp_path):
    blob = tmp_path / "camera.bin"
    blob.write_bytes(c.blob(O))
    f = _run(exe, "audit", *c.dims, c.W, c.H, repr(float(c.dt)), blob).split()
    return dict(lo=tuple(map(int, f[1:4])), hi=tuple(map(int, f[5:8])), trips=int(f[9]), fast=f[11] == "fast", accepted=f[13] == "1", overrun=f[15] == "1")


def test_narrow_field_camera_is_the_stock_camera_at_the_stock_field(O):
    for cam in ((1.0, 0.5, 1.0, (0.5, 0.5, 0.5), 1.5), FC.down_axis(0, 3.4), FC.down_axis(1, 2.0), (1020.0, 0.4, 0.7, FC.CENTRE, 2.0)):
        assert FC.narrow_blob(O, cam, 1.0) == O.camera_blob(*cam)
    # a narrowed field sees the same rays: the pixel (x, y) of a frame narrowed by 1/4 is the ray of NDC / 4
    cam = (3.0, 0.2, 0.9, FC.CENTRE, 1.0)
    wide, tele = np.frombuffer(O.camera_blob(*cam), np.float32), np.frombuffer(FC.narrow_blob(O, cam, 0.25), np.float32)
    assert (tele[:4] == wide[:4]).all() and (tele[28:36] == wide[28:36]).all() and (tele[20:28] == wide[20:28] * np.float32(0.25)).all()
    assert np.allclose(tele[4:20].reshape(4, 4).T.astype(np.float64) @ tele[20:36].reshape(4, 4).T.astype(np.float64), np.eye(4), atol=1e-3)


def test_case_list_conditions(O, fuzz_exe, tmp_path):
    cases = FC.cases()
    assert len(cases) == FC.N_CASES and len({c.name for c in cases}) == len(cases)
    sides, audits = [], {}
    for c in cases:
        assert c.W <= 32 and c.H <= 16 and c.vol.nbytes < 100_000 and c.vol.shape == c.dims[::-1], c
        eye = FC.eye_of(O, c)
        assert FC.render_accepted(c.dims, eye, c.dt), c
        fast = FC.rule_fast(c.dims, eye, c.dt, c.cell_bytes)
        # this module's rule is the header's, for every cell size and under VK_RENDER_SAFE
        for cb in (8, 16):
            assert FC.rule_fast(c.dims, eye, c.dt, cb) == _header_rule(fuzz_exe, c.dims, eye, c.dt, 0, cb), (c, cb)
        assert not _header_rule(fuzz_exe, c.dims, eye, c.dt, 4) and not FC.rule_fast(c.dims, eye, c.dt, safe_flag=True)
        sides.append(fast)
        # the volume: the long axis' first and last bricks differ from each other and from zero
        ax = c.long_axis
        line = np.moveaxis(c.vol, 2 - ax, 0).reshape(c.dims[ax], -1)[:, 0].astype(np.float32)
        assert line[0] != line[-1] and line[0] != 0 and line[-1] != 0 and (line == line[len(line) // 3]).mean() > (0.8 if len(line) >= 128 else 0.5)
        # every case the rule calls fast has passed the replay audit (every pixel of its frame)
        a = audits[c.name] = _audit(fuzz_exe, O, c, tmp_path)
        assert a["accepted"] and a["fast"] == fast, (c, a)
        if fast:
            assert not a["overrun"] and all(lo >= -2 for lo in a["lo"]) and all(hi <= n for hi, n in zip(a["hi"], c.dims)), (c, a)
    assert 3 * sum(sides) >= len(cases) and 3 * (len(cases) - sum(sides)) >= len(cases), (sum(sides), len(cases))
    by = {c.name: c for c in cases}
    # the rows overrun (a distance-only rule takes them); the budget pair sits on both sides of 16 KB; the eye pairs on both sides of their limit
    for c in cases:
        if "row" in c.tags:
            assert audits[c.name]["overrun"] and audits[c.name]["hi"][0] > c.dims[0], (c, audits[c.name])
    assert ((4079 + 4 + 4 + 9 + 3) & ~3) * 4 == 16384 and ((4080 + 4 + 4 + 9 + 3) & ~3) * 4 > 16384
    for dims in ("32x32x32", "256x8x8"):
        inside, outside = (next(c for c in cases if c.name.startswith(f"eye {s} {dims}")) for s in ("inside", "outside"))
        assert FC.rule_fast(inside.dims, FC.eye_of(O, inside), inside.dt) and not FC.rule_fast(outside.dims, FC.eye_of(O, outside), outside.dt)
    for c in cases:
        if "over" in c.tags or "fast" in c.tags:
            assert sides[cases.index(c)] == ("fast" in c.tags), c
    # the other families' cases: a long axis and a far camera on each side of the rule, a fast u8 one among them (so PACKED_PAIRS runs
    # unclamped too), and a fast u16 one
    fam = FC.family_cases()
    side = {c.name: sides[cases.index(c)] for c in fam}
    assert all(c.name in by for c in fam)
    for far in (False, True):
        group = [c for c in fam if ("eye" in c.tags) == far]
        assert any(side[c.name] for c in group) and not all(side[c.name] for c in group), (far, side)
        assert any(side[c.name] and c.kind == "u8" for c in group), (far, side)
    assert any(side[c.name] and c.u16 for c in fam)
    # R16_UNORM: a row, and both sides of the rule
    u16 = [c for c in cases if c.u16]
    assert any("row" in c.tags for c in u16) and any(sides[cases.index(c)] for c in u16) and not all(sides[cases.index(c)] for c in u16)
    assert all(int(c.vol.max()) == 257 * 30 and c.vol.dtype == np.uint16 for c in u16)
    blobs, far, W, H = FC.batch_cameras(O)
    eyes = [np.frombuffer(b, np.float32)[:3] for b in blobs]
    assert [FC.rule_fast((32, 32, 32), e, 1.0) for e in eyes] == [i != far for i in range(5)]
    assert max(range(5), key=lambda i: float(np.linalg.norm(eyes[i].astype(np.float64)))) == far


@pytest.fixture(scope="module")
def tf_lib(O, tmp_path_factory):
    return tf_helpers.build_restatement(tmp_path_factory.mktemp("fastpath_tf"), O)


def references(O, tf_lib, c):
    """The C references of a case: the oracle's built-in frame and the table restatement's -- ((rgb, steps), (rgb, steps))."""
    cam = c.blob(O)
    if c.u16:  # (the oracle and the table restatement have no R16_UNORM: the numpy references on the u16 scale, as tests/test_u16_gpu.py)
        return _u16_references(cam, c.name)
    ref, steps, _ = O.render(cam, c.vol, c.W, c.H, dt_scale=c.dt)
    tref, tsteps = tf_helpers.restate(tf_lib, O, cam, c.vol, c.W, c.H, dt=c.dt, table=FC.table(), domain=FC.DOMAIN)
    return (ref[..., :3], steps), (tref[..., :3], tsteps)


@functools.lru_cache(maxsize=None)
def _u16_references(cam, name):
    c = next(c for c in FC.cases() if c.name == name)
    ref, steps, _ = NU.render_builtin(cam, c.vol, c.W, c.H, dt=c.dt)
    tref, tsteps = NU.render_table(None, cam, c.vol, c.W, c.H, table=FC.table(), domain=FC.DOMAIN, dt=c.dt)
    return (ref, steps), (tref, tsteps)


def rel_err(got, ref):
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.maximum(1.0, np.abs(ref.astype(np.float64)))


def test_references_step_and_agree_with_numpy_on_the_shorter_cases(O, tf_lib):
    compared, twins, worst = 0, 0, (0.0, None)
    for c in FC.cases():
        (ref, steps), (tref, tsteps) = references(O, tf_lib, c)
        assert (steps == tsteps).all(), c
        assert (steps > 0).mean() >= 0.02, (c, float((steps > 0).mean()))  # at least 2 % of a case's pixels step
        assert np.isfinite(ref).all() and np.isfinite(tref).all(), c
        assert ref.max() > 0 and tref.max() > 0, c                          # ... and something shows
        if c.u16:  # numpy references already: held to the C references of the u8 twin, whose rays are the same rays
            (_, steps8), (_, tsteps8) = references(O, tf_lib, dataclasses.replace(c, u16=False))
            assert (steps == steps8).all() and (tsteps == tsteps8).all(), c
            twins += 1
            continue
        if int(steps.max()) > FC.TRIPS_NUMPY:
            continue
        cam = c.blob(O)
        got, gsteps, _ = NB.render(cam, c.vol, c.W, c.H, dt=c.dt)
        tgot, tgsteps = NR.render(cam, c.vol, c.W, c.H, table=FC.table(), domain=FC.DOMAIN, dt=c.dt)
        assert (gsteps == steps).all() and (tgsteps == tsteps).all(), c
        for e in (float(rel_err(got, ref).max()), float(rel_err(tgot, tref).max())):
            assert e <= TOL, (c, e)
            if e >= worst[0]:
                worst = (e, c.name)
        compared += 1
    assert compared >= 12 and twins == 4, (compared, twins)
    print(f"\nfastpath cases: numpy references vs C references on {compared} cases of at most {FC.TRIPS_NUMPY} trips; largest colour error {worst[0]:.3g} ({worst[1]})")


def test_bench_configurations_keep_the_unclamped_build(O, fuzz_exe):
    """The configuration bench.py times on a cell layout -- C2: 256^3 u8, dt_scale DT_SCALE, the bonsai camera and its orbits -- read from
    bench.py; C4 and C5 (1024^3 f16, 2048^3 u8) are staged volumes, which this rule does not dispatch."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    dt = float(re.search(r"^DT_SCALE\s*=\s*([\d.]+)", src, re.M).group(1))
    n = int(re.search(r'"c2": dict\(n=(\d+), fmt="u8"', src).group(1))
    assert (n, dt) == (256, 0.5)
    cams = re.findall(r"V\.Camera\(1\.0, (0\.5(?: \+ 0\.1 \* \(\(i \* B \+ j\) % 7\) / 7\.0)?), 1\.0(?: \+ 6\.28318 \* [^,]+)?, \(0\.5, 0\.5, 0\.5\), W / H\)", src)
    assert len(cams) >= 5  # the bonsai camera, its orbit by yaw, and the orbit whose pitch rises to 0.6
    for pitch in (0.5, 0.6):
        for yaw in np.linspace(0.0, 6.28318, 33) + 1.0:
            eye = np.frombuffer(O.camera_blob(1.0, pitch, float(yaw), (0.5, 0.5, 0.5), 1920 / 1080), np.float32)[:3]
            for cb in (8, 16):
                assert FC.rule_fast((n, n, n), eye, dt, cb), (pitch, yaw)
    eye = np.frombuffer(O.camera_blob(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), 1920 / 1080), np.float32)[:3]
    assert _header_rule(fuzz_exe, (n, n, n), eye, dt, 0, 8) and _header_rule(fuzz_exe, (n, n, n), eye, dt, 0, 16)
