"""The division-free block map the kernels run (vokselis_amd/csrc/vk_hostmath.hpp: udiv, block_map_make, and the overloads of
batch_block_split, deal_pos and tile_pixel that take the launch's reciprocals) against the '/'-based functions of the same header, under
AddressSanitizer and UndefinedBehaviorSanitizer on the CPU: tests/block_map_fuzz.cpp, a program of its own, run directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_map_under_sanitizers(tmp_path):
    exe = str(tmp_path / "block_map_fuzz")
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "block_map_fuzz.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "20261019"], capture_output=True, text=True, timeout=1500, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("block_map_fuzz: OK") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # the share of the argument space that sampling leaves out is stated, part by part
    assert all(("%-6s" % part) in r.stdout and "left out by sampling" in r.stdout for part in ("recip", "split", "deal", "pixel"))

