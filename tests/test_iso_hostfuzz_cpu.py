"""Host fuzz of the isosurface's shared header (vk_iso.hpp: iso_cell_empty, iso_hit, iso_k, iso_desc, iso_refine), plain g++ under ASan +
UBSan (tests/iso_fuzz.cpp), run as a program of its own: no sample of an empty cell hits, a cell with a non-finite tap is never empty,
the validation accepts exactly what the header says, and the bisection's a is that of a literal enumeration."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("iso_fuzz") / "iso_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "iso_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15"])
def test_empty_cells_hold_no_hit_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "100000", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    bad = r.stdout.split("bad ")[1].split(" of ")[0]
    empty = int(r.stdout.split("(")[-1].split(" empty")[0])
    nonfinite = int(r.stdout.split(", ")[-1].split(" non-finite")[0])
    assert bad == "0" and empty > 10000 and nonfinite > 5000, r.stdout  # (the fuzz must actually reach empty and non-finite cells)
