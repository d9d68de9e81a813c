"""Gradient lighting of the table march (vk_set_lighting) on the CPU: the shade and the parameter checks (vokselis_amd/csrc/vk_light.hpp)
fuzzed under ASan + UBSan, the C restatement of the lit march (tests/lit_restatement.c) held to the unlit table restatement, its gradient
held to central differences of the oracle's trilinear sample, and the host's light normalisation."""
import os
import subprocess

import numpy as np
import pytest

import tf_helpers
from lit_helpers import ROOT, build_restatement, light_vector, restate, sample, sphere_u8
from tf_helpers import band_pass_table, zero_band_table


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lit_fuzz") / "lit_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "lit_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15"])
def test_shade_is_finite_and_exact_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "100000", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    bad, nograd = r.stdout.split("bad ")[1].split(" of ")[0], r.stdout.split("(")[-1].split(" without")[0]
    assert bad == "0" and int(nograd) > 1000, r.stdout  # (the fuzz must actually reach the no-gradient branch)


@pytest.mark.parametrize("d", [(1.0, 2.0, 3.0), (0.0, 0.0, -1.0), (1e-30, 0.0, 1e-30), (3e38, 3e38, -1.0), (0.1, 0.7, 0.3)])
def test_light_normalisation_matches_the_library(fuzz_exe, d):
    r = subprocess.run([fuzz_exe, "light", *map(repr, d)], capture_output=True, text=True, timeout=60, check=True)
    lib = [float.fromhex(v) for v in r.stdout.split()]
    assert lib == [float(v) for v in light_vector(d)[:3]]


@pytest.fixture(scope="module")
def L(O, tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("lit_restatement"), O)


@pytest.fixture(scope="module")
def T(O, tmp_path_factory):
    return tf_helpers.build_restatement(tmp_path_factory.mktemp("tf_restatement_for_lit"), O)


@pytest.mark.parametrize("vname,cname,dt", [("standin", "bonsai_1x1", 1.0), ("standin", "inside", 0.5), ("fog", "bonsai_1x1", 0.5),
                                            ("checker", "axis", 1.0), ("ramp_x", "inside", 1.0)])
def test_identity_lighting_is_the_unlit_table(L, T, O, golden_volumes, cameras, vname, cname, dt):
    """ka = 1, kd = ks = 0: the lit restatement gives the table restatement's frame and steps bit for bit, under any light."""
    vol = golden_volumes[vname]
    for table in (zero_band_table(), band_pass_table()):
        ref, ref_steps = tf_helpers.restate(T, O, cameras[cname], vol, 64, 64, dt=dt, table=table)
        assert ref_steps.max() > 0
        for light in (light_vector("headlight", 1.0, 0.0, 0.0, 32.0), light_vector((0.3, -1.0, 0.2), 1.0, 0.0, 0.0, 1.0)):
            rgba, steps = restate(L, O, cameras[cname], vol, 64, 64, dt=dt, table=table, light=light)
            assert (rgba.view(np.uint32) == ref.view(np.uint32)).all() and (steps == ref_steps).all(), vname
        unlit, unlit_steps = restate(L, O, cameras[cname], vol, 64, 64, dt=dt, table=table)
        assert (unlit.view(np.uint32) == ref.view(np.uint32)).all() and (unlit_steps == ref_steps).all()


def test_f16_identity_lighting_is_the_unlit_table(L, T, O, cameras):
    vol = O.volume_fog_f16(32)
    ref, ref_steps = tf_helpers.restate(T, O, cameras["bonsai_1x1"], vol, 64, 64, dt=0.5, table=zero_band_table(), domain=(0.0, 1.2))
    rgba, steps = restate(L, O, cameras["bonsai_1x1"], vol, 64, 64, dt=0.5, table=zero_band_table(), domain=(0.0, 1.2),
                          light=light_vector((1.0, 1.0, 0.0), 1.0, 0.0, 0.0))
    assert (rgba.view(np.uint32) == ref.view(np.uint32)).all() and (steps == ref_steps).all()


def _random_f16(shape, rng):
    return (rng.standard_normal(shape) * 2.0).astype(np.float16)


@pytest.mark.parametrize("kind,dims", [("u8", (16, 16, 16)), ("u8", (24, 10, 7)), ("f16", (12, 12, 12)), ("f16", (9, 20, 5))])
def test_gradient_is_the_derivative_of_the_trilinear_sample(L, kind, dims):
    """Inside a cell the trilinear interpolant is linear along each axis: a central difference of vo_sample_trilinear across a fraction of
    the cell is its derivative, up to the rounding of the two samples.  World units: u = p n - 0.5, so d/dp = n d/du."""
    rng = np.random.default_rng(0x11687 + dims[0])
    nx, ny, nz = dims
    vol = rng.integers(0, 256, (nz, ny, nx), dtype=np.uint8) if kind == "u8" else _random_f16((nz, ny, nx), rng)
    n = np.array([nx, ny, nz], np.float64)
    worst = 0.0
    for _ in range(300):
        cell = rng.integers(0, n - 1)  # interior cells: both taps of every axis are real voxels
        frac = rng.uniform(0.2, 0.8, 3)
        p = np.float32((cell + frac + 0.5) / n)
        v, g = sample(L, vol, p)
        scale = max(1.0, float(np.abs(g).max()))
        for a in range(3):
            h = np.float32(0.1 / n[a])
            pp, pm = p.copy(), p.copy()
            pp[a] = np.float32(p[a] + h)
            pm[a] = np.float32(p[a] - h)
            fp, _ = sample(L, vol, pp)
            fm, _ = sample(L, vol, pm)
            cd = (float(fp) - float(fm)) / (float(pp[a]) - float(pm[a]))
            err = abs(cd - float(g[a])) / scale
            worst = max(worst, err)
            assert err < 1e-3, (kind, dims, cell, frac, a, cd, g)
    assert worst > 0.0 or kind == "u8"


def test_sphere_normals_point_along_the_radius(L):
    """On a ball the gradient of the density points to the centre, whatever the voxel aspect (the world scaling of g)."""
    for dims in ((48, 48, 48), (64, 32, 24)):
        vol = sphere_u8(*dims)
        for p in ((0.85, 0.5, 0.5), (0.5, 0.16, 0.5), (0.5, 0.5, 0.86), (0.7, 0.7, 0.3)):  # (in the shell, r ~ 0.35)
            _, g = sample(L, vol, p)
            r = np.array(p) - 0.5
            cos = float(np.dot(-g, r) / (np.linalg.norm(g) * np.linalg.norm(r)))
            assert cos > 0.98, (dims, p, g, cos)
