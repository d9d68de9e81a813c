"""The host side of the volume histogram (vk_volume_histogram, vk_histogram_window) without a GPU: the C boundary (the
two exports, the 16-byte vk_histogram, the 24-byte vk_voxel_box and the 72-byte vk_volume_stats in include/vokselis_hip.h, sizeof from a
compiled C snippet, the ABI number unchanged), the host-callable pieces of vokselis_amd/csrc/vk_hist.hpp against brute force under ASan +
UBSan (tests/hist_fuzz.cpp, a stand-alone program), vk_histogram_window through the library (it needs no context), the Python surface, and
the argument refusals of the C++ host's bonsai --histogram / --auto-window."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("vk_volume_histogram", "vk_histogram_window")


def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_exports_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert re.search(r"#define\s+VK_HIST_MAX_BINS\s+4096\b", code) and re.search(r"enum \{ VK_HIST_CLIP_BOX = 1 \};", code)
    assert re.search(r"typedef struct vk_histogram \{\s*float lo, hi;\s*uint32_t bins;\s*uint32_t flags;\s*\} vk_histogram;", code)
    assert re.search(r"typedef struct vk_voxel_box \{\s*uint32_t x0, y0, z0, x1, y1, z1;\s*\} vk_voxel_box;", code)
    assert re.search(r"typedef struct vk_volume_stats \{\s*uint64_t n_voxels, n_nan, n_below, n_above, n_finite;\s*double sum, sum_sq;\s*float min, max;\s*float scale;\s*uint32_t pad;\s*\} vk_volume_stats;", code)
    for decl in (r"int vk_volume_histogram\(vk_ctx \*ctx, const vk_histogram \*hist, const vk_voxel_box \*box, uint64_t \*counts, vk_volume_stats \*stats\);",
                 r"int vk_histogram_window\(const uint64_t \*counts, uint32_t bins, float lo, float hi, double p_lo, double p_hi, float \*w_lo, float \*w_hi\);"):
        assert re.search(decl, code), decl
    for phrase in ("Each voxel is counted once, whatever the layout duplicates", "the top is closed, like numpy.histogram's", "-0 at lo_k = 0 is bin 0",
                   "changes no context", "counts == bincount(v >> 8)", "no float atomics"):
        assert phrase in _header(), phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 20\. ", design, flags=re.M) and "vk_volume_histogram" in design and "-0 at lo_k = 0 is bin 0" in design


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_hist.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(vk_histogram), offsetof(vk_histogram, bins), offsetof(vk_histogram, flags), '
                   'sizeof(vk_voxel_box), offsetof(vk_voxel_box, x1), sizeof(vk_volume_stats), offsetof(vk_volume_stats, n_finite), offsetof(vk_volume_stats, sum), '
                   'offsetof(vk_volume_stats, min), offsetof(vk_volume_stats, scale), VK_ABI_VERSION, VK_HIST_MAX_BINS, VK_HIST_CLIP_BOX); return 0; }\n')
    exe = tmp_path / "sizeof_hist"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["16", "8", "12", "24", "12", "72", "32", "40", "56", "64", "5", "4096", "1"], out


def test_library_exports_answer_a_null_context_with_an_error(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert C.sizeof(N.VkHistogram) == 16 and [f[0] for f in N.VkHistogram._fields_] == ["lo", "hi", "bins", "flags"]
    assert C.sizeof(N.VkVoxelBox) == 24 and [f[0] for f in N.VkVoxelBox._fields_] == ["x0", "y0", "z0", "x1", "y1", "z1"]
    assert C.sizeof(N.VkVolumeStats) == 72 and [f[0] for f in N.VkVolumeStats._fields_] == ["n_voxels", "n_nan", "n_below", "n_above", "n_finite", "sum", "sum_sq", "min", "max", "scale", "pad"]
    for name in EXPORTS:
        assert N.SYMBOLS[name][0] is C.c_int and getattr(hip_built, name)
    req, st = N.VkHistogram(0.0, 1.0, 4, 0), N.VkVolumeStats()
    counts = (C.c_uint64 * 4)(9, 9, 9, 9)
    st.n_voxels = 77
    assert hip_built.vk_volume_histogram(None, C.byref(req), None, counts, C.byref(st)) == -1
    assert list(counts) == [9, 9, 9, 9] and st.n_voxels == 77


def _window(lib, counts, lo, hi, p_lo, p_hi):
    c = np.ascontiguousarray(counts, np.uint64)
    a, b = C.c_float(-1.0), C.c_float(-2.0)
    rc = lib.vk_histogram_window(c.ctypes.data_as(C.POINTER(C.c_uint64)), len(c), lo, hi, p_lo, p_hi, C.byref(a), C.byref(b))
    return rc, a.value, b.value


def test_histogram_window_needs_no_context(hip_built):
    counts = [1, 2, 0, 5]
    assert _window(hip_built, counts, 0.0, 1.0, 0.0, 1.0) == (0, 0.0, 1.0)
    assert _window(hip_built, counts, 0.0, 1.0, 0.5, 1.0) == (0, 0.75, 1.0)      # r_lo = 4: the running totals 1, 3, 3, 8 exceed it in bin 3
    assert _window(hip_built, counts, 0.0, 1.0, 0.0, 0.125) == (0, 0.0, 0.25)    # r_hi = 1: reached in bin 0
    assert _window(hip_built, counts, 0.0, 1.0, 0.125, 0.375) == (0, 0.25, 0.5)  # r_lo = 1 exceeded in bin 1; r_hi = 3 reached in bin 1
    assert _window(hip_built, counts, -2.0, 2.0, 0.2, 0.3) == (0, -1.0, 0.0)
    for bad in ((0.5, 0.5), (0.9, 0.1), (-0.1, 0.5), (0.1, 1.5), (float("nan"), 0.5)):
        rc, a, b = _window(hip_built, counts, 0.0, 1.0, *bad)
        assert (rc, a, b) == (-1, -1.0, -2.0), bad
        assert b"vk_histogram_window" in hip_built.vk_last_error(None)
    assert _window(hip_built, [0, 0, 0], 0.0, 1.0, 0.1, 0.9)[0] == -1 and b"empty" in hip_built.vk_last_error(None)
    assert _window(hip_built, counts, 1.0, 1.0, 0.1, 0.9)[0] == -1
    big = float(np.float32(1e30))
    assert _window(hip_built, counts, big, float(np.nextafter(np.float32(1e30), np.float32(np.inf))), 0.0, 0.1)[0] == -1  # w_lo >= w_hi once rounded
    assert hip_built.vk_histogram_window(None, 4, 0.0, 1.0, 0.1, 0.9, C.byref(C.c_float()), C.byref(C.c_float())) == -1


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd import _native as N
    from vokselis_amd.context import Context

    assert (V.HIST_MAX_BINS, V.HIST_CLIP_BOX) == (4096, 1)
    for name in ("HIST_MAX_BINS", "HIST_CLIP_BOX", "VkHistogram", "VkVoxelBox", "VkVolumeStats", "Histogram"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.volume_histogram)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("bins", 256), ("domain", (0.0, 1.0)), ("box", None)]
    assert "vk_volume_histogram" in Context.volume_histogram.__doc__ and "vk_histogram_window" in V.Histogram.window.__doc__
    st = N.VkVolumeStats()
    st.n_voxels, st.n_nan, st.n_below, st.n_above, st.n_finite = 10, 1, 2, 3, 8
    st.sum, st.sum_sq, st.min, st.max, st.scale = 255.0 * 4.0, 255.0 * 255.0 * 4.0, 0.0, 255.0, 255.0   # eight texels: four of 0, four of 255
    h = V.Histogram(np.array([3, 1], np.uint64), (0.0, 1.0), st)
    assert (h.n_voxels, h.n_nan, h.n_below, h.n_above, h.n_finite, h.bins) == (10, 1, 2, 3, 8, 2)
    assert h.counts.dtype == np.uint64 and list(h.edges) == [0.0, 0.5, 1.0]
    assert (h.min, h.max, h.mean, h.std) == (0.0, 1.0, 0.5, 0.5)
    st.n_finite = 0
    e = V.Histogram(np.zeros(2, np.uint64), (0.0, 1.0), st)
    assert np.isnan(e.mean) and np.isnan(e.std)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hist_fuzz") / "hist_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "hist_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261019"])
def test_validation_bins_keys_boxes_window_flush_and_grid_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "400", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (400 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.fixture(scope="module")
def bonsai():
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(ROOT, "vokselis_amd", "_lib", "bonsai")
    assert os.path.exists(exe)
    return exe


@pytest.mark.parametrize("args, message", [
    (["--histogram", "0"], "BINS lies in 1 .. 4096"),
    (["--histogram", "4097"], "BINS lies in 1 .. 4096"),
    (["--histogram", "16", "2", "1"], "LO and HI must be finite, LO < HI"),
    (["--histogram", "16", "nan", "1"], "LO and HI must be finite, LO < HI"),
    (["--histogram", "16", "0.5"], "LO needs HI"),
    (["--histogram"], "missing value for --histogram"),
    (["--histogram", "16", "--slice", "z", "0.5"], "--histogram replaces the render"),
    (["--histogram", "16", "--gpus", "2"], "--histogram replaces the render"),
    (["--auto-window", "0.01", "0.99"], "needs a mode that has a window"),
    (["--auto-window", "0.01", "0.99", "--iso", "0.5"], "needs a mode that has a window"),
    (["--auto-window", "0.9", "0.1", "--mip"], "needs 0 <= P_LO < P_HI <= 1"),
    (["--auto-window", "0.5", "0.5", "--mip"], "needs 0 <= P_LO < P_HI <= 1"),
    (["--auto-window", "-0.1", "0.5", "--mip"], "needs 0 <= P_LO < P_HI <= 1"),
    (["--auto-window", "0.1", "1.5", "--slice", "z", "0.5"], "needs 0 <= P_LO < P_HI <= 1"),
    (["--auto-window", "0.01", "0.99", "--mip", "--gpus", "2"], "--auto-window runs on one GPU"),
    (["--auto-window", "0.01", "0.99", "--mip", "--histogram", "16"], "--histogram replaces the render"),
    (["--auto-window", "0.01"], "missing value for --auto-window"),
])
def test_bonsai_refuses_bad_histogram_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
