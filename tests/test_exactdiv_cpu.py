"""The short divisions of the cell march's ray set-up (vokselis_amd/csrc/vk_exactdiv.hpp) on the CPU, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/exactdiv_fuzz.cpp holds them to IEEE division."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vokselis_amd", "csrc")


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("exactdiv") / "exactdiv_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "exactdiv_fuzz.cpp")], check=True)
    return exe


def test_exactdiv_under_sanitizers(fuzz_exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    out = r.stdout
    assert out.strip().endswith("OK") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # div_const, exhaustively up to 16384: sum of W; the identity's and the chain's case counts as the program states them
    assert "const: %d cases" % (16384 * 16385 // 2) in out and "pow2: 30000000 cases" in out and "50000000 random pairs" in out
    # the one seed-dependent case the chain has on the CPU: 1 / 0x1.fffffep0 from the bracket below the true reciprocal
    listed = re.findall(r"seed-dependent: (\S+) / (\S+) with seed (\S+)", out)
    assert listed == [("0x1p+0", "0x1.fffffep+0", "0x1p-1")], listed


def test_the_kernels_take_the_header_under_test():
    """The kernel body calls the functions the fuzz includes and keeps the generic text beside them."""
    body = open(os.path.join(CSRC, "vk_march_kernel_body.hpp")).read()
    for name in ("div_const(", "recip_refine(", "div_by(", "div_inrange(", "pow2_recip(", "LF_SETUP_GENERIC", "kDivLo", "kDivHi"):
        assert name in body, name
    assert "normalize3(dir[0], dir[1], dir[2]);" in body and "1.0f / (fnx * fabsf(dir[0]))" in body  # the generic text stays
    common = open(os.path.join(CSRC, "vk_common.hpp")).read()
    assert "float rcp_w, rcp_h;" in common
