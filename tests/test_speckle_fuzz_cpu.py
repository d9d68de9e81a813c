"""The lone-speckle code of the built-in skip maps (vk_tf.hpp: speckle_code, speckle_proven) on the CPU: a host fuzz under ASan + UBSan
(tests/speckle_fuzz.cpp) over every hot value 26..255 against every cold maximum 0..25 in all eight corners, at adversarial and random
weights.  Proven implies alpha == +0 on the filter chains of both u8 cell layouts, the encoder agrees with an integer restatement and
codes nothing but single-hot u8 cells, and the stand-in's range comes out proven for at least a quarter of its samples."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("speckle_fuzz") / "speckle_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "speckle_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15"])
def test_speckle_code_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "32", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    line = r.stdout.strip().splitlines()[-1]
    bad, proven = line.split("bad ")[1].split(" of ")[0], int(line.split("(")[1].split(" proven")[0])
    sp, sn = (int(x) for x in line.split("stand-in range ")[1].split(" proven")[0].split(" of "))
    print("\n" + line)
    assert bad == "0", line
    assert proven > 1000000, line  # (the fuzz must actually reach proven samples)
    assert 4 * sp >= sn, line      # non-vacuity: a quarter of the stand-in's range at the least
