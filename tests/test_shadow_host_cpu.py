"""The host side of light-direction shadows (vk_set_shadows) without a GPU: the C boundary (the two exports and the
8-byte struct in include/vokselis_hip.h, the ABI number unchanged), the validation and the host-callable pieces of
vokselis_amd/csrc/vk_shadow.hpp against brute force under ASan + UBSan (tests/shadow_fuzz.cpp, a stand-alone program), and the Python
surface."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_exports_and_the_struct_and_keeps_the_abi_number():
    hdr = _header()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert re.search(r"#define\s+VK_SHADOW_MAX_BIAS\s+1024\b", code)
    assert re.search(r"typedef struct vk_shadows \{\s*float strength;\s*float bias;\s*\} vk_shadows;", code)
    assert re.search(r"int vk_set_shadows\(vk_ctx \*ctx, const vk_shadows \*s\);", code)
    assert re.search(r"int vk_get_shadows\(vk_ctx \*ctx, vk_shadows \*out, int \*enabled\);", code)


def test_library_exports_answer_a_null_context_with_an_error(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert C.sizeof(N.VkShadows) == 8 and [f[0] for f in N.VkShadows._fields_] == ["strength", "bias"]
    assert N.SYMBOLS["vk_set_shadows"][0] is C.c_int and N.SYMBOLS["vk_get_shadows"][0] is C.c_int
    s = N.VkShadows(0.7, 2.0)
    on = C.c_int(5)
    assert hip_built.vk_set_shadows(None, None) == -1 and hip_built.vk_set_shadows(None, C.byref(s)) == -1
    assert hip_built.vk_get_shadows(None, C.byref(s), C.byref(on)) == -1 and on.value == 5


def test_python_surface():
    from vokselis_amd.context import Context

    sig = inspect.signature(Context.set_shadows)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("strength", 0.7), ("bias", 2.0)]
    assert isinstance(Context.shadows, property)
    doc = Context.set_shadows.__doc__
    assert "vk_set_shadows" in doc and "None" in doc and "headlight" in doc


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shadow_fuzz") / "shadow_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "shadow_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261021"])
def test_validation_table_ts0_and_k_under_sanitizers(fuzz_exe, seed):
    """Every refused value leaves the descriptor as it was; ts0 and k are what brute force gives."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "400", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (400 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
