"""The runtime transfer function (vk_set_transfer_function) on the CPU: the emptiness predicate the skip maps are rebuilt with
(vokselis_amd/csrc/vk_tf.hpp) fuzzed under ASan + UBSan against the march's own filter and lookup, the C restatement of the march under
a table (tests/tf_restatement.c) held to the oracle on the golden case, and the Python table helper."""
import os
import subprocess

import numpy as np
import pytest

from tf_helpers import ROOT, band_pass_table, build_restatement, restate, tf_constants, zero_band_table


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tf_fuzz") / "tf_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "tf_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15"])
def test_empty_cells_sample_zero_alpha_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "100000", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    bad, empty = r.stdout.split("bad ")[1].split(" of ")[0], r.stdout.split("(")[-1].split(" empty")[0]
    assert bad == "0" and int(empty) > 1000, r.stdout  # (the fuzz must actually reach empty cells)


@pytest.fixture(scope="module")
def L(O, tmp_path_factory):
    return build_restatement(tmp_path_factory.mktemp("tf_restatement"), O)


@pytest.mark.parametrize("vname,cname,dt", [("standin", "bonsai_1x1", 1.0), ("standin", "inside", 0.5), ("fog", "bonsai_1x1", 0.5),
                                            ("checker", "axis", 1.0), ("ramp_x", "inside", 1.0), ("impulse", "bonsai_1x1", 1.0)])
def test_restatement_builtin_branch_is_the_oracle(L, O, golden, golden_volumes, cameras, vname, cname, dt):
    """The restatement's loop with the built-in transfer reproduces vo_render bit for bit (and the golden fixture)."""
    vol = golden_volumes[vname]
    rgba, steps = restate(L, O, cameras[cname], vol, 64, 64, dt=dt)
    ref, ref_steps, _ = O.render(cameras[cname], vol, 64, 64, dt_scale=dt)
    assert (rgba.view(np.uint32) == ref.view(np.uint32)).all()
    assert (steps == ref_steps).all()
    key = f"{vname}__{cname}__dt{dt}"
    g = golden["naive_64x64"]
    assert (steps == g[key + "__steps"]).all()
    assert float(np.abs(rgba - g[key + "__rgba"]).max()) <= 1e-6


def test_restatement_f16_builtin_branch_is_the_oracle(L, O, golden, cameras):
    vol = O.volume_fog_f16(32)
    rgba, steps = restate(L, O, cameras["bonsai_1x1"], vol, 64, 64, dt=0.5)
    ref, ref_steps, _ = O.render(cameras["bonsai_1x1"], vol, 64, 64, dt_scale=0.5)
    assert (rgba.view(np.uint32) == ref.view(np.uint32)).all() and (steps == ref_steps).all()
    assert (steps == golden["naive_f16_64x64"]["steps"]).all()


def test_restatement_table_branch(L, O, golden_volumes, cameras):
    """A transparent table leaves every ray black and marching to its end; an opaque table ends every hit ray within two steps;
    misses stay the clear colour whatever the table."""
    vol = golden_volumes["standin"]
    cam = cameras["bonsai_1x1"]
    clear = np.zeros((256, 4), np.float32)
    clear[:, :3] = 1.0
    rgba, steps = restate(L, O, cam, vol, 64, 64, table=clear)
    assert (rgba[..., :3] == 0).all() and (rgba[..., 3] == 1).all()
    _, ref_steps, _ = O.render(cam, np.zeros_like(vol), 64, 64, dt_scale=1.0)  # (an empty volume: every ray marches to its end)
    assert (steps == ref_steps).all()
    hit = steps > 0
    rgba_o, steps_o = restate(L, O, cam, vol, 64, 64, table=np.ones((2, 4), np.float32))
    assert (steps_o[hit] <= 2).all() and (steps_o[~hit] == 0).all() and (rgba_o[hit][:, :3] > 0.9).all()
    rgba_b, steps_b = restate(L, O, cam, vol, 64, 64, table=band_pass_table())
    assert np.isfinite(rgba_b).all() and (steps_b[~hit] == 0).all() and (rgba_b[~hit][:, :3] == 0).all()


@pytest.mark.parametrize("n,lo,hi,r8", [(2, -1.0, 3.0, 0), (256, 0.1, 0.6, 1), (256, 0.0, 1.0, 1), (17, 0.3, 0.30001, 0), (200, -2.5, 7.25, 1),
                                         (256, 0.1, 0.1000001, 1)])
def test_table_constants_match_the_library(fuzz_exe, n, lo, hi, r8):
    """k1 = (n-1) / ((hi-lo) S) and k2 = -lo (n-1) / (hi-lo), in double, each rounded once to f32: the library's vk_tf.hpp (through the
    fuzz binary) and the restatement's helper give the same bits, and both are the once-rounded values."""
    r = subprocess.run([fuzz_exe, "constants", str(n), repr(lo), repr(hi), str(r8)], capture_output=True, text=True, timeout=60, check=True)
    k1_lib, k2_lib = (float.fromhex(v) for v in r.stdout.split())
    lo32, hi32 = np.float32(lo), np.float32(hi)
    assert (k1_lib, k2_lib) == tf_constants(n, lo32, hi32, bool(r8))
    span = float(hi32) - float(lo32)
    assert k1_lib == float(np.float32((n - 1) / (span * (255.0 if r8 else 1.0)))) and k2_lib == float(np.float32(-float(lo32) * (n - 1) / span))


def test_transfer_table_is_piecewise_linear():
    import vokselis_amd as V

    t = V.transfer_table([(0.5, 1, 0, 0, 1), (0.0, 0, 0, 1, 0)], n=5)
    assert t.dtype == np.float32 and t.shape == (5, 4)
    assert np.allclose(t[:, 3], [0, 0.5, 1, 1, 1]) and np.allclose(t[:, 0], [0, 0.5, 1, 1, 1]) and np.allclose(t[:, 2], [1, 0.5, 0, 0, 0])
    assert (zero_band_table()[:26, 3] == 0).all() and (zero_band_table()[26:, 3] > 0).all()
    with pytest.raises(ValueError):
        V.transfer_table([(0, 1, 1, 1)], n=4)
    with pytest.raises(ValueError):
        V.transfer_table([(0, 1, 1, 1, 1)], n=257)
