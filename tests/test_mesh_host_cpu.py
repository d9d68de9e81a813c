"""The host side of the mesh pass (vk_extract_isosurface) without a GPU: the C boundary (the export, the 8-byte
vk_mesh_request in include/vokselis_hip.h, sizeof from a compiled C snippet, the ABI number unchanged), the host-callable pieces of
vokselis_amd/csrc/vk_mesh.hpp against brute force under ASan + UBSan (tests/mesh_fuzz.cpp, a stand-alone program), the Python surface,
weld / write_stl / write_obj on a known tetrahedron, and the argument refusals of the C++ host's bonsai --mesh."""
import ctypes as C
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_struct_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert re.search(r"enum \{ VK_MESH_CLIP_BOX = 1 \};", code)
    assert re.search(r"typedef struct vk_mesh_request \{\s*float iso;\s*uint32_t flags;\s*\} vk_mesh_request;", code)
    assert re.search(r"int vk_extract_isosurface\(vk_ctx \*ctx, const vk_mesh_request \*req, const vk_voxel_box \*box, float \*triangles, uint64_t cap_triangles, uint64_t \*n_triangles\);", code)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 21\. ", design, flags=re.M) and "vk_extract_isosurface" in design
    for phrase in ("a true divide", "(01,23,03) (01,12,23)", "x fastest, then y, then z", "bitwise prefix", "changes no context state", "v >= iso_k"):
        assert phrase in _header(), phrase
    for phrase in ("a true divide", "(01,23,03) (01,12,23)", "Out of scope"):
        assert phrase in design[design.index("## 21. "):], phrase
    assert "vk_extract_isosurface" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_sizeof_the_struct_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_mesh.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %d\\n", sizeof(vk_mesh_request), offsetof(vk_mesh_request, iso), offsetof(vk_mesh_request, flags), '
                   'VK_ABI_VERSION, VK_MESH_CLIP_BOX); return 0; }\n')
    exe = tmp_path / "sizeof_mesh"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["8", "0", "4", "5", "1"], out


def test_library_export_answers_a_null_context_with_an_error(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert C.sizeof(N.VkMeshRequest) == 8 and [f[0] for f in N.VkMeshRequest._fields_] == ["iso", "flags"]
    assert N.SYMBOLS["vk_extract_isosurface"][0] is C.c_int and hip_built.vk_extract_isosurface
    req, n = N.VkMeshRequest(0.5, 0), C.c_uint64(77)
    tris = (C.c_float * 9)(*([3.5] * 9))
    assert hip_built.vk_extract_isosurface(None, C.byref(req), None, tris, 1, C.byref(n)) == -1
    assert n.value == 77 and list(tris) == [3.5] * 9


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context

    assert V.MESH_CLIP_BOX == 1
    for name in ("MESH_CLIP_BOX", "VkMeshRequest", "weld", "write_stl", "write_obj"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.extract_isosurface)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("iso", inspect.Parameter.empty), ("box", None), ("max_triangles", None)]
    assert "vk_extract_isosurface" in Context.extract_isosurface.__doc__
    assert [p.name for p in inspect.signature(V.write_stl).parameters.values()] == ["path", "tris", "scale"]


def _tetrahedron():
    """The tetrahedron (0,0,0), (1,0,0), (0,1,0), (0,0,1) with outward normals: four triangles, four vertices, six edges."""
    o, x, y, z = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    return np.array([[o, y, x], [o, x, z], [o, z, y], [x, y, z]], np.float32)


def test_weld_merges_by_bit_pattern_in_order_of_first_use():
    import vokselis_amd as V

    tris = _tetrahedron()
    verts, faces = V.weld(tris)
    assert verts.dtype == np.float32 and verts.tolist() == [[0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1]]
    assert faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 1], [2, 1, 3]]
    assert (verts[faces].view(np.uint32) == tris.view(np.uint32)).all()
    signed = tris.copy()
    signed[1, 0, 0] = -0.0  # -0 is another pattern than +0
    assert len(V.weld(signed)[0]) == 5
    e, f = V.weld(np.zeros((0, 3, 3), np.float32))
    assert e.shape == (0, 3) and f.shape == (0, 3)
    with pytest.raises(ValueError):
        V.weld(np.zeros((4, 3), np.float32))


def test_write_stl_round_trips_the_tetrahedron(tmp_path):
    import vokselis_amd as V

    tris = _tetrahedron()
    path = tmp_path / "t.stl"
    assert V.write_stl(str(path), tris, scale=(2.0, 3.0, 4.0)) == 4
    raw = path.read_bytes()
    assert len(raw) == 80 + 4 + 4 * 50 and struct.unpack("<I", raw[80:84])[0] == 4
    rec = np.frombuffer(raw[84:], np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")]))
    assert (rec["v"] == tris * np.array([2.0, 3.0, 4.0], np.float32)).all() and not rec["attr"].any()
    assert rec["n"][:3].tolist() == [[0, 0, -1], [0, -1, 0], [-1, 0, 0]]
    want = np.array([12.0, 8.0, 6.0]) / np.sqrt(12.0 ** 2 + 8.0 ** 2 + 6.0 ** 2)  # the plane x / 2 + y / 3 + z / 4 = 1
    assert (rec["n"][3] == want.astype(np.float32)).all()
    flat = np.zeros((1, 3, 3), np.float32)  # a triangle without area: the zero normal
    V.write_stl(str(path), flat)
    assert not np.frombuffer(path.read_bytes()[84:], np.float32, 12).any()


def test_write_obj_round_trips_the_tetrahedron(tmp_path):
    import vokselis_amd as V

    tris = _tetrahedron() * np.float32(1.0 / 3.0)  # coordinates that need all nine digits
    path = tmp_path / "t.obj"
    assert V.write_obj(str(path), tris) == (4, 4)
    v, f = [], []
    for line in path.read_text().splitlines():
        if line.startswith("v "):
            v.append([float(t) for t in line.split()[1:]])
        elif line.startswith("f "):
            f.append([int(t) - 1 for t in line.split()[1:]])
    v, f = np.array(v, np.float32), np.array(f)
    assert v.shape == (4, 3) and f.shape == (4, 3)
    assert (v[f].view(np.uint32) == tris.view(np.uint32)).all()


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_fuzz") / "mesh_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "mesh_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261019"])
def test_table_fraction_mapping_scan_and_validation_under_sanitizers(fuzz_exe, seed):
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
    (["--mesh", "out.stl"], "--mesh needs an isovalue"),
    (["--mesh", "out.obj", "--mip"], "--mesh needs an isovalue"),
    (["--mesh", "out.ply", "--iso", "0.3"], "ends in .stl or .obj"),
    (["--mesh", "stl", "--iso", "0.3"], "ends in .stl or .obj"),
    (["--mesh"], "missing value for --mesh"),
    (["--mesh-iso", "0.3"], "--mesh-iso and --mesh-scale need --mesh"),
    (["--mesh-scale", "1", "2", "3", "--iso", "0.3"], "--mesh-iso and --mesh-scale need --mesh"),
    (["--mesh", "out.stl", "--mesh-iso", "nan"], "V must be finite"),
    (["--mesh", "out.stl", "--mesh-iso", "inf"], "V must be finite"),
    (["--mesh", "out.stl", "--iso", "nan"], "the isovalue must be finite"),
    (["--mesh", "out.stl", "--mesh-iso", "0.3", "--mesh-scale", "1", "0", "1"], "finite and > 0"),
    (["--mesh", "out.stl", "--mesh-iso", "0.3", "--mesh-scale", "1", "2"], "missing value for --mesh-scale"),
    (["--mesh", "out.stl", "--iso", "0.3", "--histogram", "16"], "--mesh replaces the render"),
    (["--mesh", "out.stl", "--iso", "0.3", "--slice", "z", "0.5"], "--mesh replaces the render"),
    (["--mesh", "out.obj", "--mesh-iso", "0.3", "--gpus", "2"], "--mesh replaces the render"),
])
def test_bonsai_refuses_bad_mesh_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
