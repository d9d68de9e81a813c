"""The two references of vk_distance_transform held together over the shared cases (tests/dist_cases.py): the C
restatement (tests/dist_restatement.c: a quadratic minimum along every line) and the numpy reference (tests/np_dist_reference.py) --
squared distances, morphed volume and counts, bit for bit; both against the distance by its definition on the small volumes and against
scipy.ndimage.distance_transform_edt where scipy imports.  The conditions on the case list are asserted, so the list cannot quietly
degenerate.  The host side -- the C boundary, vk_dist.hpp under ASan + UBSan (tests/dist_fuzz.cpp, a stand-alone program), the Python
surface, bonsai's argument handling -- needs no GPU either."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dist_cases as DC
import dist_helpers as DH
import label_helpers as LH
import np_dist_reference as ND
import np_label_reference as NL

ROOT = DH.ROOT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return DH.build_restatement(tmp_path_factory.mktemp("dist_fuzz_cpu"))


@pytest.fixture(scope="module")
def restated(lib):
    return {c.name: DH.restate_case(lib, c) for c in DC.cases()}


def test_case_list_covers_the_issue(restated):
    cases = DC.cases()
    assert len({c.name for c in cases}) == len(cases) and 300 <= len(cases) <= 600, len(cases)
    assert max(c.vol.size for c in cases) <= DC.MAX_VOXELS
    src = open(os.path.join(ROOT, "vokselis_amd", "csrc", "vk_launch_dist.hip")).read()
    assert int(re.search(r"kDistThreads = (\d+);", src).group(1)) == DC.WORKGROUP and int(re.search(r"kDistTile = (\d+),", src).group(1)) == DC.TILE
    dims = {tuple(reversed(c.vol.shape)) for c in cases}
    assert dims == set(DC.DIMS) | set(DC.LONG) | {DC.REFUSED}
    assert {(1, 1, 1), (70, 1, 1), (1, 70, 1), (1, 1, 70), (300, 3, 2), (2, 300, 3), (3, 2, 300), (37, 21, 11), (48, 40, 33)} <= dims
    assert all(n <= 3 or (n % DC.WAVE and n % DC.TILE) for d in dims for n in d)                   # no dimension is a multiple of the wave (so of the workgroup) or of the transpose's tile
    assert any(d[0] > DC.TILE and d[1] > DC.TILE for d in dims) and all(any(d[a] > 2 * DC.TILE for d in dims) for a in (0, 1))  # tiles side by side along x and y at once; more than two along each
    assert all(any(d[a] > DC.WORKGROUP for d in dims) and any(DC.WAVE < d[a] < DC.WORKGROUP for d in dims) for a in range(3))  # lines longer than a wave, than a workgroup
    for kind in ("u8", "u16", "f16"):
        mine = [c for c in cases if c.kind == kind]
        text = " | ".join(c.name for c in mine)
        for word in ("empty", "full", "one voxel in the middle", "two voxels at opposite corners", "a plane", "density 0.05", "density 0.31", "density 0.7", "porous block with a gap",
                     "joined by a bridge", ", box (", "clip box", "empty box", "uniform noise") + tuple("one voxel at corner %d" % k for k in range(8)):
            assert word in text, (kind, word)
        assert {c.op for c in mine} == set(ND.OPS) and {c.spacing for c in mine} == set(DC.SPACINGS)
        assert {c.radius for c in mine if c.op in DC.MORPH and c.spacing == (1, 1, 1)} >= set(DC.RADII)
        for d in DC.DIMS + DC.LONG:
            assert {c.op for c in mine if tuple(reversed(c.vol.shape)) == d} >= {"outside", "inside"}, (kind, d)
        assert sum(c.refused for c in mine) == 1
    special = [c for c in cases if "NaN, inf" in c.name]
    assert {(c.lo, c.hi) for c in special} >= {(-math.inf, math.inf), (math.inf, math.inf), (-math.inf, -math.inf), (0.0, 0.0)}
    # what the cases exercise, on the restatement's output
    assert all((restated[c.name] is None) == c.refused for c in cases)
    assert any(1000.0 ** 2 > sum((s * (n - 1)) ** 2 for s, n in zip(c.spacing, reversed(c.vol.shape))) for c in cases if c.radius == 1000.0)  # a radius larger than the volume
    bounds = [sum((s * (n - 1)) ** 2 for s, n in zip(c.spacing, reversed(c.vol.shape))) for c in cases]
    assert any(2 ** 31 < b <= 0xFFFFFFFE for b in bounds) and sum(b > 0xFFFFFFFE for b in bounds) == 3
    assert max(int(r[2][4]) for r in restated.values() if r is not None) == (64 * 899) ** 2 > 2 ** 31                             # max_d2 above 2^31
    off_axis = 0
    for c in cases:
        r = restated[c.name]
        if r is not None and r[0] is not None and c.spacing == (1, 1, 1):
            finite = r[0][r[0] != ND.INF].astype(np.int64)
            off_axis += bool((np.sqrt(finite).round() ** 2 != finite).any())                                                     # a D2 no single axis attains (2, 3, 5 ...)
    assert off_axis > 20
    empty = restated[next(c.name for c in cases if c.kind == "u8" and "empty, " in c.name and c.op == "outside")]
    full = restated[next(c.name for c in cases if c.kind == "u8" and " full, " in c.name and c.op == "inside")]
    assert (empty[0] == ND.INF).all() and (full[0] == ND.INF).all() and int(empty[2][4]) == 0 and int(full[2][0]) == full[0].size


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(restated):
    for c in DC.cases():
        assert DH.differences(restated[c.name], DH.reference_case(c)) == "", c.name


def test_both_agree_with_the_distance_by_its_definition_on_the_small_volumes(restated):
    done = 0
    for c in DC.cases():
        small_set = not c.refused and c.kind == "u8" and c.vol.size <= 9000 and c.op in ("outside", "dilate") and int(restated[c.name][2][0]) <= 1000
        if c.refused or not (c.vol.size <= 2500 or small_set):  # (all pairs: the volumes of up to 2500 voxels, and the sparse sets on the next larger one)
            continue
        assert DH.differences(restated[c.name], DH.reference_case(c, d2=ND.brute)) == "", c.name
        done += 1
    assert done > 120, done


def test_both_agree_with_scipy_where_the_target_set_is_not_empty(restated):
    ndimage = pytest.importorskip("scipy.ndimage")
    done = 0
    for c in DC.cases():
        if c.op not in ("outside", "inside") or c.refused:
            continue
        s = NL.foreground(c.vol, c.kind, c.lo, c.hi, c.box)
        target = s if c.op == "outside" else ~s
        if not target.any():
            continue
        want = np.rint(ndimage.distance_transform_edt(~target, sampling=c.spacing[::-1]) ** 2).astype(np.uint32)
        assert (want == restated[c.name][0]).all() and (want == ND.d2_to(target, c.spacing)).all(), c.name
        done += 1
    assert done > 100


def test_properties_of_the_rule(restated, lib):
    cases = DC.cases()
    for c in cases:
        r = restated[c.name]
        if r is None:
            continue
        s = NL.foreground(c.vol, c.kind, c.lo, c.hi, c.box)
        assert int(r[2][0]) == int(s.sum()), c.name
        if c.op in ("outside", "inside"):
            assert ((r[0] == 0) == (s if c.op == "outside" else ~s)).all() and int(r[2][1]) == int(s.sum()) and not r[2][2:4].any(), c.name
            continue
        kept, F_in, F_out = LH.raw(r[1]), LH.raw(NL.fill_bits(c.fill_in, c.kind).reshape(1))[0], LH.raw(NL.fill_bits(c.fill_out, c.kind).reshape(1))[0]
        orig = LH.raw(c.vol)
        assert ((kept == orig) | (~s & (kept == F_in)) | (s & (kept == F_out))).all(), c.name                 # a voxel keeps its bits or takes its side's fill
        assert int(r[2][1]) == int(r[2][0]) + int(r[2][2]) - int(r[2][3]) and int(r[2][4]) == 0, c.name
        if c.radius == 0.0:
            assert (kept == orig).all() and int(r[2][1]) == int(r[2][0]) and not r[2][2:4].any(), c.name       # radius 0: all four ops return S
        if c.op in ("close", "dilate"):
            assert int(r[2][3]) == 0, c.name                                                                   # CLOSE and DILATE contain S
        if c.op in ("open", "erode"):
            assert int(r[2][2]) == 0, c.name                                                                   # OPEN and ERODE are contained in S
    assert {c.op for c in cases if c.radius == 0.0 and c.op in DC.MORPH} == set(DC.MORPH)
    # CLOSE of CLOSE is CLOSE, OPEN of OPEN is OPEN: the operator applied to its own result (as a two-valued volume) changes nothing
    again = 0
    for c in cases:
        if c.op not in ("close", "open") or c.kind != "u8" or c.box is not None or c.refused or c.vol.size > 12000:
            continue
        m = ND.morph(NL.foreground(c.vol, c.kind, c.lo, c.hi, None), c.op, c.spacing, ND.r2_of(c.radius))
        twice = DH.restate(lib, DC.mask_volume(m, "u8"), "u8", 0.5, math.inf, c.op, c.spacing, c.radius, 1.0, 0.0)
        assert not twice[2][2:4].any() and int(twice[2][1]) == int(m.sum()), c.name
        again += 1
    assert again >= 8
    # CLOSE at radius 1.5 fills the pores and the gap: one component afterwards; OPEN at 1.5 cuts the bridge: two
    for kind in ("u8", "u16", "f16"):
        c = next(c for c in cases if c.kind == kind and "porous block" in c.name and c.op == "close" and c.radius == 1.5)
        before, after = NL.foreground(c.vol, kind, c.lo, c.hi, None), NL.foreground(restated[c.name][1], kind, c.lo, c.hi, None)
        assert len(NL.label(c.vol, kind, c.lo, c.hi, 6, None)[1]) == 2 and len(NL.label(restated[c.name][1], kind, c.lo, c.hi, 6, None)[1]) == 1
        block = np.zeros(before.shape, bool)
        block[2:-2, 3:-3, 4:-4] = True
        assert (after <= block).all() and after[3:-3, 4:-4, 5:-5].all() and not before[3:-3, 4:-4, 5:-5].all()             # every pore and the gap, away from the block's rim
        assert int(restated[c.name][2][2]) == int((after & ~before).sum()) > 100
        c = next(c for c in cases if c.kind == kind and "joined by a bridge" in c.name and c.op == "open" and c.radius == 1.5)
        assert len(NL.label(c.vol, kind, c.lo, c.hi, 6, None)[1]) == 1 and len(NL.label(restated[c.name][1], kind, c.lo, c.hi, 6, None)[1]) == 2


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code) and re.search(r"#define\s+VK_DIST_INF\s+0xFFFFFFFFu", code)
    assert re.search(r"#define\s+VK_DIST_MAX_SPACING\s+64\b", code) and re.search(r"#define\s+VK_DIST_MAX_RADIUS\s+65535\.0f", code)
    assert "enum { VK_DIST_OUTSIDE = 0, VK_DIST_INSIDE = 1, VK_DIST_DILATE = 2, VK_DIST_ERODE = 3, VK_DIST_CLOSE = 4, VK_DIST_OPEN = 5 };" in code
    assert "enum { VK_DIST_CLIP_BOX = 1, VK_DIST_INSTALL = 2 };" in code
    assert re.search(r"int vk_distance_transform\(vk_ctx \*ctx, const vk_distance_request \*req, const vk_voxel_box \*box, uint32_t \*d2_out, void \*dense_out,\s*"
                     r"vk_distance_result \*result\);", code)
    assert "static_assert(sizeof(vk_distance_request) == 40 && sizeof(vk_distance_result) == 40" in code
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 25\. ", design, flags=re.M)
    section = design[design.index("## 25. "):]
    for phrase in ("sum_c (spacing[c] * (v_c - u_c))^2", "R2 = (uint64_t)floor((double)radius * (double)radius)", "dil(A) = { v : D2(A, v) <= R2 }", "ero(A) = { v : D2(not A, v) > R2 }",
                   "VK_DIST_INSTALL", "0xFFFFFFFE"):
        assert phrase in _header(), phrase
        assert phrase in section, phrase
    for word in ("Loop bounds", "2 n", "Measurements"):
        assert word in section, word
    assert "vk_distance_transform" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "morph_volume" in open(os.path.join(ROOT, "README.md")).read() and "dist_quick.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "dist_pass_isa.txt"))


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_dist.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %u\\n", sizeof(vk_distance_request), offsetof(vk_distance_request, op), '
                   'offsetof(vk_distance_request, flags), offsetof(vk_distance_request, spacing), offsetof(vk_distance_request, radius), offsetof(vk_distance_request, fill_in), '
                   'offsetof(vk_distance_request, fill_out), sizeof(vk_distance_result), offsetof(vk_distance_result, n_removed), offsetof(vk_distance_result, max_d2), '
                   'VK_ABI_VERSION, VK_DIST_MAX_SPACING, VK_DIST_OPEN, VK_DIST_INSTALL, VK_DIST_INF); return 0; }\n')
    exe = tmp_path / "sizeof_dist"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["40", "8", "12", "16", "28", "32", "36", "40", "24", "32", "5", "64", "5", "2", "4294967295"], out


def test_the_binding_matches_and_every_export_resolves(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert (C.sizeof(N.VkDistanceRequest), C.sizeof(N.VkDistanceResult)) == (40, 40)
    assert [f[0] for f in N.VkDistanceRequest._fields_] == ["lo", "hi", "op", "flags", "spacing", "radius", "fill_in", "fill_out"]
    assert [f[0] for f in N.VkDistanceResult._fields_] == ["n_foreground", "n_result", "n_added", "n_removed", "max_d2", "pad"]
    assert (N.VkDistanceRequest.spacing.offset, N.VkDistanceRequest.radius.offset, N.VkDistanceRequest.fill_out.offset, N.VkDistanceResult.max_d2.offset) == (16, 28, 36, 32)
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert "vk_distance_transform" in declared and declared == set(N.SYMBOLS), declared ^ set(N.SYMBOLS)
    assert hip_built.vk_distance_transform is not None
    # a NULL context: an error, the outputs untouched
    req, res, d2 = N.VkDistanceRequest(), N.VkDistanceResult(7, 7, 7, 7, 7, 7), np.full(8, 9, np.uint32)
    assert hip_built.vk_distance_transform(None, C.byref(req), None, d2.ctypes.data, None, C.byref(res)) == -1
    assert (d2 == 9).all() and res.n_foreground == 7 and res.max_d2 == 7


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context
    from vokselis_amd.distance import default_fill_in, distance_request

    assert (V.DIST_INF, V.DIST_MAX_SPACING, V.DIST_MAX_RADIUS) == (0xFFFFFFFF, 64, 65535.0)
    assert (V.DIST_OUTSIDE, V.DIST_INSIDE, V.DIST_DILATE, V.DIST_ERODE, V.DIST_CLOSE, V.DIST_OPEN, V.DIST_CLIP_BOX, V.DIST_INSTALL) == (0, 1, 2, 3, 4, 5, 1, 2)
    for name in ("DIST_INF", "DIST_OPEN", "DIST_INSTALL", "VkDistanceRequest", "VkDistanceResult", "distance_request"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.distance_transform)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("which", "outside"), ("spacing", (1, 1, 1)), ("box", None)]
    sig = inspect.signature(Context.morph_volume)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("op", "close"), ("radius", 1.0), ("spacing", (1, 1, 1)),
                                                                             ("fill_in", None), ("fill_out", 0.0), ("install", True), ("out", False), ("box", None)]
    r = distance_request(0.3, op="open", radius=1.5, spacing=(2, 2, 5), fill_in=0.75, fill_out=0.25, install=True, box="clip")
    assert (r.lo, r.hi, r.op, r.flags, list(r.spacing), r.radius, r.fill_in, r.fill_out) == (np.float32(0.3), math.inf, 5, 3, [2, 2, 5], 1.5, 0.75, 0.25)
    r = distance_request(0.2, 0.4, op="inside")
    assert (r.op, r.flags, list(r.spacing), r.radius, r.fill_in, r.fill_out) == (1, 0, [1, 1, 1], 0.0, np.float32(0.4), 0.0)
    # the fill a voxel takes when the caller names none lies in the range once it is stored: u8 [0.3, inf) must not get 0.3 (76 < 76.5)
    assert default_fill_in(0.3, math.inf) == 1.0 and default_fill_in(2.0, math.inf) == 2.0 and default_fill_in(0.2, 0.4) == 0.4 and default_fill_in(-math.inf, math.inf) == 1.0
    for bad in (dict(op="shrink"), dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(spacing=(1, 65, 1)), dict(spacing=(1.5, 1, 1)), dict(op="close", radius=-1.0),
                dict(op="close", radius=math.nan), dict(op="close", radius=65536.0)):
        with pytest.raises(ValueError):
            distance_request(0.3, **bad)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dist_fuzz") / "dist_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "dist_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261020"])
def test_line_function_columns_bound_and_validation_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "2000", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (2000 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.fixture(scope="module")
def bonsai():
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(ROOT, "vokselis_amd", "_lib", "bonsai")
    assert os.path.exists(exe)
    return exe


NEEDS_RANGE = "--morph needs a value range: --components LO HI, or --iso V for [V, inf)"


@pytest.mark.parametrize("args, message", [
    (["--morph", "close", "1.5"], NEEDS_RANGE), (["--morph", "open", "2", "--morph-spacing", "1", "1", "2"], NEEDS_RANGE),
    (["--morph", "shrink", "1", "--iso", "0.3"], "--morph OP RADIUS: OP is close, open, dilate or erode"),
    (["--morph", "close", "-1", "--iso", "0.3"], "--morph OP RADIUS: a finite RADIUS of 0 .. 65535"), (["--morph", "close", "nan", "--iso", "0.3"], "--morph OP RADIUS: a finite RADIUS of 0 .. 65535"),
    (["--morph", "close", "70000", "--iso", "0.3"], "--morph OP RADIUS: a finite RADIUS of 0 .. 65535"),
    (["--morph", "close"], "missing value for --morph"), (["--morph-spacing", "1", "2"], "missing value for --morph-spacing"),
    (["--morph-spacing", "1", "0", "1", "--morph", "close", "1", "--iso", "0.3"], "--morph-spacing SX SY SZ: integers of 1 .. 64"),
    (["--morph-spacing", "1", "65", "1", "--morph", "close", "1", "--iso", "0.3"], "--morph-spacing SX SY SZ: integers of 1 .. 64"),
    (["--morph-spacing", "1", "1", "1", "--iso", "0.3"], "--morph-spacing needs --morph"), (["--morph-fill", "1", "0", "--iso", "0.3"], "--morph-fill needs --morph"),
    (["--morph-fill", "inf", "0", "--morph", "close", "1", "--iso", "0.3"], "--morph-fill IN OUT: finite values"),
    (["--iso", "0.3"] + ["--morph", "close", "1"] * 17, "--morph: at most 16 times"),
    (["--morph", "close", "1", "--iso", "0.3", "--gpus", "2"], "--morph runs on one GPU"),
])
def test_bonsai_refuses_bad_morph_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
