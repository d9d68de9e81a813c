"""The host side of the slice pass (vk_render_slice, vk_slice_probe) without a GPU: the C boundary (the five exports,
the 56-byte vk_slice and the 20-byte vk_slice_sample in include/vokselis_hip.h, sizeof from a compiled C snippet, the ABI number
unchanged), the host-callable pieces of vokselis_amd/csrc/vk_slice.hpp against brute force under ASan + UBSan (tests/slice_fuzz.cpp, a
stand-alone program), the Python surface with the Slice builder's vectors against hand-computed ones, and the argument refusals of the
C++ host's bonsai --slice / --slice-plane / --slab."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("vk_render_slice", "vk_slice_values_info", "vk_readback_slice_values", "vk_frame_slice_values", "vk_slice_probe")


def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_exports_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert re.search(r"typedef struct vk_slice \{\s*float origin\[3\];\s*float du\[3\];\s*float dv\[3\];\s*float dn\[3\];\s*uint32_t samples;\s*int32_t reduce;\s*\} vk_slice;", code)
    assert re.search(r"typedef struct vk_slice_sample \{\s*int32_t inside;\s*float pos\[3\];\s*float value;\s*\} vk_slice_sample;", code)
    assert re.search(r"#define\s+VK_SLICE_MAX_SAMPLES\s+256\b", code) and re.search(r"#define\s+VK_SLICE_MAX_COORD\s+1e6f\b", code)
    assert re.search(r"enum \{ VK_SLAB_MAX = 0, VK_SLAB_MIN = 1, VK_SLAB_MEAN = 2 \};", code) and re.search(r"enum \{ VK_SLICE_VALUES = 1 \};", code)
    for decl in (r"int vk_render_slice\(vk_ctx \*ctx, const vk_slice \*slice, int32_t tile_x, int32_t tile_y, uint32_t tile_w, uint32_t tile_h, uint32_t flags\);",
                 r"int vk_slice_values_info\(vk_ctx \*ctx, uint32_t \*width, uint32_t \*height, void \*\*device_ptr\);",
                 r"int vk_readback_slice_values\(vk_ctx \*ctx, void \*dst, size_t row_pitch_bytes\);",
                 r"int vk_frame_slice_values\(vk_ctx \*ctx, uint64_t frame_id, void \*dst, size_t row_pitch_bytes\);",
                 r"int vk_slice_probe\(vk_ctx \*ctx, const vk_slice \*slice, uint32_t x, uint32_t y, vk_slice_sample \*out\);"):
        assert re.search(decl, code), decl
    for phrase in ("vk_render_partition, vk_render_batch, vk_group_render and the fused present have no slice output", "no inside test per sample",
                   "a pixel's result never depends on the tile"):
        assert phrase in _header(), phrase


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_slice.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(vk_slice), offsetof(vk_slice, du), offsetof(vk_slice, dv), '
                   'offsetof(vk_slice, dn), offsetof(vk_slice, samples), offsetof(vk_slice, reduce), sizeof(vk_slice_sample), offsetof(vk_slice_sample, pos), '
                   'offsetof(vk_slice_sample, value), VK_ABI_VERSION, VK_SLICE_MAX_SAMPLES); return 0; }\n')
    exe = tmp_path / "sizeof_slice"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["56", "12", "24", "36", "48", "52", "20", "4", "16", "5", "256"], out


def test_library_exports_answer_a_null_context_with_an_error(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert C.sizeof(N.VkSlice) == 56 and [f[0] for f in N.VkSlice._fields_] == ["origin", "du", "dv", "dn", "samples", "reduce"]
    assert C.sizeof(N.VkSliceSample) == 20 and [f[0] for f in N.VkSliceSample._fields_] == ["inside", "pos", "value"]
    for name in EXPORTS:
        assert N.SYMBOLS[name][0] is C.c_int and getattr(hip_built, name)
    s, o = N.VkSlice(), N.VkSliceSample()
    buf = (C.c_float * 8)()
    w = C.c_uint32(7)
    assert hip_built.vk_render_slice(None, C.byref(s), 0, 0, 8, 8, 0) == -1
    assert hip_built.vk_slice_values_info(None, C.byref(w), None, None) == -1 and w.value == 7
    assert hip_built.vk_readback_slice_values(None, buf, 32) == -1
    assert hip_built.vk_frame_slice_values(None, 1, buf, 32) == -1
    assert hip_built.vk_slice_probe(None, C.byref(s), 0, 0, C.byref(o)) == -1


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context

    assert (V.SLAB_MAX, V.SLAB_MIN, V.SLAB_MEAN, V.SLICE_VALUES, V.SLICE_MAX_SAMPLES) == (0, 1, 2, 1, 256)
    for name in ("SLAB_MAX", "SLAB_MIN", "SLAB_MEAN", "SLICE_VALUES", "SLICE_MAX_SAMPLES", "VkSlice", "VkSliceSample", "Slice"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.render_slice)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("slice", inspect.Parameter.empty), ("tile", None), ("values", False)]
    assert [p for p in inspect.signature(Context.read_slice_values).parameters] == ["self"]
    assert [p for p in inspect.signature(Context.frame_slice_values).parameters][1:] == ["frame_id"]
    assert [p for p in inspect.signature(Context.slice_probe).parameters][1:] == ["slice", "x", "y"]
    assert "vk_render_slice" in Context.render_slice.__doc__ and "vk_slice_probe" in Context.slice_probe.__doc__
    sig = inspect.signature(V.Slice.plane)
    assert [p.name for p in sig.parameters.values()] == ["centre", "normal", "up", "width", "height", "extent", "thickness", "samples", "reduce", "spacing", "dims"]
    assert (sig.parameters["thickness"].default, sig.parameters["samples"].default, sig.parameters["reduce"].default, sig.parameters["spacing"].default) == (0.0, 1, "max", (1.0, 1.0, 1.0))
    for fn in (V.Slice.axial, V.Slice.coronal, V.Slice.sagittal):
        assert [p.name for p in inspect.signature(fn).parameters.values()][:4] == ["dims", "index", "width", "height"]


def _vec(s):
    return [list(s.origin), list(s.du), list(s.dv), list(s.dn)]


def _f32(rows):
    return [[float(np.float32(v)) for v in r] for r in rows]


def test_slice_builder_against_hand_computed_vectors():
    import vokselis_amd as V

    # a 4 x 2 frame one cube wide, facing +z, y up: pixels a quarter apart; pixel (0, 0)'s centre 1.5 pixels left of and half a pixel above the centre
    s = V.Slice.plane((0.5, 0.5, 0.5), (0, 0, 1), (0, 1, 0), 4, 2, 1.0)
    assert _vec(s) == [[0.125, 0.625, 0.5], [0.25, 0.0, 0.0], [0.0, -0.25, 0.0], [0.0, 0.0, 0.0]] and (s.samples, s.reduce) == (1, V.SLAB_MAX)
    assert all(np.signbit(np.float32(v)) == (v < 0) for row in _vec(s) for v in row)  # no -0 component
    # an `up` that leans into the normal is made perpendicular; a slab of 5 planes over 0.2: 0.05 apart along the normal
    s = V.Slice.plane((0.5, 0.5, 0.5), (0, 0, 2), (0, 3, 7), 4, 2, 1.0, thickness=0.2, samples=5, reduce="mean")
    assert _vec(s) == _f32([[0.125, 0.625, 0.5], [0.25, 0.0, 0.0], [0.0, -0.25, 0.0], [0.0, 0.0, 0.05]]) and (s.samples, s.reduce) == (5, V.SLAB_MEAN)
    # facing +x, z up: +x on screen is z x x = +y
    s = V.Slice.plane((0.25, 0.5, 0.5), (1, 0, 0), (0, 0, 1), 8, 8, 0.5, reduce="min")
    assert _vec(s) == _f32([[0.25, 0.5 - 3.5 / 16, 0.5 + 3.5 / 16], [0.0, 1 / 16, 0.0], [0.0, 0.0, -1 / 16], [0.0, 0.0, 0.0]]) and s.reduce == V.SLAB_MIN
    # spacing / dims: a 100 x 100 x 50 volume of unit spacing is half as thick in z: a pixel 0.01 of the longest side is 0.01 in x and 0.02 in z
    s = V.Slice.plane((0.5, 0.5, 0.5), (0, 1, 0), (0, 0, 1), 100, 50, 1.0, dims=(100, 100, 50))
    assert _vec(s)[1:3] == _f32([[-0.01, 0.0, 0.0], [0.0, 0.0, -0.02]])
    assert _vec(s)[0] == _f32([[0.5 + 49.5 * 0.01, 0.5, 0.5 + 24.5 * 0.02]])[0]
    # ... and so is a 100^3 volume whose z spacing is half the others'
    t = V.Slice.plane((0.5, 0.5, 0.5), (0, 1, 0), (0, 0, 1), 100, 50, 1.0, spacing=(1.0, 1.0, 0.5), dims=(100, 100, 100))
    assert _vec(t) == _vec(s)
    # the orthogonal views put pixel centres on texel centres where the sizes match
    s = V.Slice.axial((16, 8, 4), 2, 16, 8)
    assert _vec(s) == [[1 / 32, 1 / 16, 2.5 / 4], [1 / 16, 0.0, 0.0], [0.0, 1 / 8, 0.0], [0.0, 0.0, 1 / 4]]
    s = V.Slice.coronal((16, 8, 4), 3, 16, 4, samples=3, reduce="mean")
    assert _vec(s) == [[1 / 32, 3.5 / 8, 1 / 8], [1 / 16, 0.0, 0.0], [0.0, 0.0, 1 / 4], [0.0, 1 / 8, 0.0]] and (s.samples, s.reduce) == (3, V.SLAB_MEAN)
    s = V.Slice.sagittal((16, 8, 4), 5, 8, 4)
    assert _vec(s) == [[5.5 / 16, 1 / 16, 1 / 8], [0.0, 1 / 8, 0.0], [0.0, 0.0, 1 / 4], [1 / 16, 0.0, 0.0]]
    # what the builder refuses before the library sees it
    for bad in (dict(samples=0), dict(samples=257), dict(reduce="median"), dict(extent=0.0), dict(extent=float("nan")), dict(normal=(0, 0, 0)), dict(up=(0, 0, 5))):
        kw = dict(centre=(0.5, 0.5, 0.5), normal=(0, 0, 1), up=(0, 1, 0), width=4, height=2, extent=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            V.Slice.plane(**kw)
    with pytest.raises(ValueError):
        V.Slice.raw((0, 0, float("inf")), (1, 0, 0), (0, 1, 0))
    with pytest.raises(ValueError):
        V.Slice.raw((0, 0, 0), (2e6, 0, 0), (0, 1, 0))
    assert V.Slice.raw((1e6, 0, 0), (-1e6, 0, 0), (0, 1, 0)).origin[0] == 1e6


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slice_fuzz") / "slice_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "slice_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261019"])
def test_validation_rn_offsets_position_and_readback_arithmetic_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "300", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (300 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.fixture(scope="module")
def bonsai():
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(ROOT, "vokselis_amd", "_lib", "bonsai")
    assert os.path.exists(exe)
    return exe


@pytest.mark.parametrize("args, message", [
    (["--slice", "w", "0.5"], "AXIS is x, y or z"),
    (["--slice", "z", "1.5"], "POS lies in 0 .. 1"),
    (["--slice", "z", "-0.1"], "POS lies in 0 .. 1"),
    (["--slice", "z", "nan"], "POS lies in 0 .. 1"),
    (["--slice", "z", "0.5", "--slice-plane", "0.5", "0.5", "0.5", "0", "0", "1", "1"], "exclude each other"),
    (["--slice-plane", "0.5", "0.5", "0.5", "0", "0", "0", "1"], "the normal has no direction"),
    (["--slice-plane", "0.5", "0.5", "0.5", "0", "0", "1", "0"], "EXTENT must be finite and > 0"),
    (["--slab", "8", "0.1", "mean"], "--slab needs --slice or --slice-plane"),
    (["--slice", "x", "0.5", "--slab", "0", "0.1", "mean"], "SAMPLES lies in 1 .. 256"),
    (["--slice", "x", "0.5", "--slab", "257", "0.1", "max"], "SAMPLES lies in 1 .. 256"),
    (["--slice", "x", "0.5", "--slab", "8", "-1", "max"], "THICKNESS must be finite and >= 0"),
    (["--slice", "x", "0.5", "--slab", "8", "0.1", "median"], "the reduction is max, min or mean"),
    (["--slice", "y", "0.5", "--gpus", "2"], "render on one GPU"),
    (["--slice", "y", "0.5", "--dump-rgba", "/dev/null"], "replace the raycast"),
    (["--slice", "y"], "missing value for --slice"),
])
def test_bonsai_refuses_bad_slice_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
