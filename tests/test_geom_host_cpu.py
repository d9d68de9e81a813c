"""The host side of the geometry pass of the first-hit isosurface (vk_render_geometry, vk_pick) without a GPU: the C
boundary (the five exports and the 36-byte vk_hit in include/vokselis_hip.h, sizeof from a compiled C snippet, the ABI number unchanged),
the host-callable pieces of vokselis_amd/csrc/vk_geom.hpp against brute force under ASan + UBSan (tests/geom_fuzz.cpp, a stand-alone
program), and the Python surface."""
import ctypes as C
import dataclasses
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("vk_render_geometry", "vk_geometry_info", "vk_readback_geometry", "vk_frame_geometry", "vk_pick")


def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_exports_and_the_struct_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert re.search(r"typedef struct vk_hit \{\s*int32_t hit;\s*float pos\[3\];\s*float t;\s*float grad\[3\];\s*float value;\s*\} vk_hit;", code)
    for decl in (r"int vk_render_geometry\(vk_ctx \*ctx, int32_t tile_x, int32_t tile_y, uint32_t tile_w, uint32_t tile_h, float dt_scale, uint32_t flags\);",
                 r"int vk_geometry_info\(vk_ctx \*ctx, uint32_t \*width, uint32_t \*height, void \*\*device_ptr\);",
                 r"int vk_readback_geometry\(vk_ctx \*ctx, void \*dst, size_t row_pitch_bytes\);",
                 r"int vk_frame_geometry\(vk_ctx \*ctx, uint64_t frame_id, void \*dst, size_t row_pitch_bytes\);",
                 r"int vk_pick\(vk_ctx \*ctx, uint32_t x, uint32_t y, float dt_scale, vk_hit \*out\);"):
        assert re.search(decl, code), decl
    # the header says what the pass does not reach, the normal's convention and the cut face's gradient
    for phrase in ("vk_render_partition, vk_render_batch, vk_group_render and the fused present have no geometry output", "-g / |g|", "not the face's normal"):
        assert phrase in _header(), phrase


def test_sizeof_vk_hit_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_hit.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d\\n", sizeof(vk_hit), offsetof(vk_hit, pos), offsetof(vk_hit, t), offsetof(vk_hit, grad), '
                   'offsetof(vk_hit, value), VK_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizeof_hit"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["36", "4", "16", "20", "32", "5"], out


def test_library_exports_answer_a_null_context_with_an_error(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert C.sizeof(N.VkHit) == 36 and [f[0] for f in N.VkHit._fields_] == ["hit", "pos", "t", "grad", "value"]
    for name in EXPORTS:
        assert N.SYMBOLS[name][0] is C.c_int and getattr(hip_built, name)
    h = N.VkHit()
    buf = (C.c_float * 8)()
    w = C.c_uint32(7)
    assert hip_built.vk_render_geometry(None, 0, 0, 8, 8, 1.0, 0) == -1
    assert hip_built.vk_geometry_info(None, C.byref(w), None, None) == -1 and w.value == 7
    assert hip_built.vk_readback_geometry(None, buf, 32) == -1
    assert hip_built.vk_frame_geometry(None, 1, buf, 32) == -1
    assert hip_built.vk_pick(None, 0, 0, 1.0, C.byref(h)) == -1


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context

    sig = inspect.signature(Context.render_geometry)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("dt_scale", 1.0), ("tile", None), ("flags", 0)]
    sig = inspect.signature(Context.pick)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("x", inspect.Parameter.empty), ("y", inspect.Parameter.empty), ("dt_scale", 1.0)]
    assert [p for p in inspect.signature(Context.frame_geometry).parameters][1:] == ["frame_id"]
    assert [p for p in inspect.signature(Context.read_geometry).parameters] == ["self"]
    assert "vk_render_geometry" in Context.render_geometry.__doc__ and "vk_pick" in Context.pick.__doc__ and "None" in Context.pick.__doc__
    assert V.Hit is V.context.Hit and "Hit" in V.__all__ and dataclasses.is_dataclass(V.Hit)
    assert [f.name for f in dataclasses.fields(V.Hit)] == ["pos", "t", "grad", "value", "normal"]


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geom_fuzz") / "geom_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "geom_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261022"])
def test_flags_distance_miss_record_and_readback_arithmetic_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "300", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (300 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
