"""The two references of vk_local_thickness held together over the shared cases (tests/thick_cases.py): the C
restatement (tests/thick_restatement.c: every voxel of the set paints its ball) and the numpy reference (tests/np_thick_reference.py:
level by level, largest first) -- T2, dense array and totals, bit for bit; the three properties that follow from the rule; the fixed
case with its pinned numbers.  The conditions on the case list are asserted, so the list cannot quietly degenerate.  The host side --
the C boundary, vk_thick.hpp under ASan + UBSan (tests/thick_fuzz.cpp, a stand-alone program), the Python surface, bonsai's argument
handling -- needs no GPU either."""
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
import np_label_reference as NL
import np_thick_reference as NT
import thick_cases as TC
import thick_helpers as TH

ROOT = TH.ROOT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return TH.build_restatement(tmp_path_factory.mktemp("thick_fuzz_cpu"))


@pytest.fixture(scope="module")
def dist_lib(tmp_path_factory):
    return DH.build_restatement(tmp_path_factory.mktemp("thick_fuzz_cpu_dist"))


@pytest.fixture(scope="module")
def restated(lib):
    return {c.name: TH.restate_case(lib, c) for c in TC.cases()}


def _dims(c):
    return tuple(reversed(c.vol.shape))


def test_case_list_covers_the_issue(restated):
    cases = TC.cases()
    assert len({c.name for c in cases}) == len(cases) and 120 <= len(cases) <= 200, len(cases)
    assert max(c.vol.size for c in cases) <= TC.MAX_VOXELS
    src = open(os.path.join(ROOT, "vokselis_amd", "csrc", "vk_thick.hpp")).read()
    assert int(re.search(r"kThickTile = (\d+),", src).group(1)) == TC.TILE
    dims = {_dims(c) for c in cases}
    assert set(TC.DIMS) | {(37, 21, 11), (48, 40, 33)} == dims
    assert all(any(d[a] == 1 for d in dims) for a in range(3))                                              # 1 on each axis
    assert {7, 9, 17, 33, 70} <= {n for d in dims for n in d} and all(n % TC.TILE for d in TC.DIMS for n in d)  # extents that are no multiple of the tile (48 and 40 are: a tile that ends on the border)
    assert any(all(n > 2 * TC.TILE for n in d) for d in dims)                                               # 3 x 3 x 3 tiles or more: a walk crosses tiles on every side
    for kind in ("u8", "u16", "f16"):
        mine = [c for c in cases if c.kind == kind]
        text = " | ".join(c.name for c in mine)
        for word in ("empty", "full", "one voxel at the far corner", "a plate 2 thick", "a plate 5 thick", "a wedge", "two overlapping balls", "balls cut by the border",
                     "porous block with a gap", "density 0.31", "density 0.9", ", box (", "clip box", "empty box", "uniform noise"):
            assert word in text, (kind, word)
        assert {c.spacing for c in mine} == set(TC.SPACINGS)
        assert {c.gain == 0.0 for c in mine} == {True, False}                                               # automatic and fixed gain
        assert any(c.max_radius / min(c.spacing) == 32.0 and c.vol.size < 10000 for c in mine)              # the largest allowed reach on a small volume
        # the cap below, at and above the largest D
        balls = [(c, restated[c.name]) for c in mine if "two overlapping balls" in c.name and c.spacing == (1, 1, 1)]
        caps = sorted(NT.cap_of(c.max_radius) for c, _ in balls)
        assert caps == [36, 100, 101, 1024] and [int(r[2][1]) for c, r in sorted(balls, key=lambda p: p[0].max_radius)] == [36, 100, 101, 101]
    special = [c for c in cases if "NaN, inf" in c.name]
    assert {(c.lo, c.hi) for c in special} >= {(-math.inf, math.inf), (math.inf, math.inf), (-math.inf, -math.inf), (0.0, 0.0)}
    # what the cases exercise, on the restatement's output
    assert all(r is not None for r in restated.values())
    distinct = {c.name: len(np.unique(restated[c.name][0])) for c in cases}
    assert max(v for k, v in distinct.items() if "a wedge" in k) >= 15                                      # many distinct T2
    empty = restated[next(c.name for c in cases if c.kind == "u8" and "empty, " in c.name)]
    full = next(c for c in cases if c.kind == "u8" and " full, " in c.name and c.max_radius == 32.0)
    assert not empty[0].any() and not empty[2][:4].any() and int(empty[2][4]) == 0                          # the empty set: nothing, and the automatic gain is 0
    assert (restated[full.name][0] == 1024).all() and int(restated[full.name][2][2]) == full.vol.size      # the full volume: every voxel C
    raised = sum(bool((restated[c.name][0].astype(np.int64) > NT.capped_distance(NL.foreground(c.vol, c.kind, c.lo, c.hi, c.box), c.spacing, NT.cap_of(c.max_radius))).any())
                 for c in cases if c.kind == "u8")
    assert raised > 20                                                                                      # T2 above Dc: a neighbour's ball is the larger one


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(restated):
    for c in TC.cases():
        assert TH.differences(restated[c.name], TH.reference_case(c)) == "", c.name


def test_properties_of_the_rule(restated, lib, dist_lib):
    cases = TC.cases()
    opened = larger = 0
    for c in cases:
        t2, dense, result = restated[c.name]
        s = NL.foreground(c.vol, c.kind, c.lo, c.hi, c.box)
        cap = NT.cap_of(c.max_radius)
        dc = NT.capped_distance(s, c.spacing, cap)
        # 1. T2 = 0 off S, Dc <= T2 <= min(max D, C) on S; no INF anywhere
        assert not t2[~s].any() and int(result[0]) == int(s.sum()), c.name
        if s.any():
            assert (t2[s] >= dc[s]).all() and (dc[s] > 0).all() and int(t2.max()) == int(dc.max()) <= cap and int(result[1]) == int(t2.max()), c.name
        assert int(result[2]) == int((t2 == cap).sum()) and int(result[3]) == int(t2.astype(np.uint64).sum()), c.name
        fill = LH.raw(NL.fill_bits(c.fill_out, c.kind).reshape(1))[0]
        assert (LH.raw(dense)[~s] == fill).all(), c.name
        if c.kind != "u8" or c.vol.size > 20000 and c.spacing != (1, 1, 1):
            continue
        # 2. for every R2 < C, VK_DIST_OPEN at R2 is contained in { T2 > R2 }: OPEN from the distance pass's restatement
        for r2 in sorted({0, 1, 2, cap // 2, cap - 1} - {cap}):
            if r2 < 0 or r2 >= cap or r2 > 400:
                continue
            radius = math.sqrt(r2 + 0.5)
            assert int(math.floor(float(np.float32(radius)) ** 2)) == r2
            leave = 0.0 if c.lo > 0.0 else 1.0  # a value outside [lo, hi] (asserted below): a voxel of S that leaves takes it, and so differs from what it stored
            assert not NL.foreground(np.full((1, 1, 1), NL.fill_bits(leave, c.kind)), c.kind, c.lo, c.hi, None).any()
            o = DH.restate(dist_lib, c.vol, c.kind, c.lo, c.hi, "open", c.spacing, radius, 1.0, leave, c.box)
            kept = s & (LH.raw(o[1]) == LH.raw(np.ascontiguousarray(c.vol)))  # OPEN is contained in S
            assert int(o[2][1]) == int(kept.sum()), c.name
            assert (t2[kept].astype(np.int64) > r2).all(), (c.name, r2)
            opened += 1
        # 3. where the result at a larger cap is <= C the result at cap C equals it; elsewhere it is <= C
        if c.max_radius / min(c.spacing) <= 16.0:
            big = TH.restate(lib, c.vol, c.kind, c.lo, c.hi, c.spacing, c.max_radius * 2.0, c.gain, c.fill_out, c.box)[0]
            below = big <= cap
            assert (t2[below] == big[below]).all() and (t2 <= cap).all() and (t2[~below] <= cap).all(), c.name
            larger += 1
    assert opened > 60 and larger > 15, (opened, larger)


def test_the_fixed_case_gives_the_pinned_numbers(lib):
    d, A, B = TC.fixed_case()
    assert d == (40, 32, 24)
    vol = DC.mask_volume(A | B, "u8")
    assert int((A | B).sum()) == 3586 and int((B & ~A).sum()) == 515
    for spacing, max_radius, top, at_top, distinct, b_only in (((1, 1, 1), 32.0, 82, 3071, 2, 26), ((1, 1, 1), 6.0, 36, 3017, 3, 26), ((1, 1, 2), 32.0, 82, 1565, 13, None)):
        for got in (TH.restate(lib, vol, "u8", 0.5, math.inf, spacing, max_radius), NT.apply(vol, "u8", 0.5, math.inf, spacing, max_radius, 0.0, 0.0, None)):
            t2 = got[0]
            assert int(got[2][0]) == 3586 and int(t2.max()) == top == int(got[2][1]) and int((t2 == top).sum()) == at_top and len(np.unique(t2[t2 > 0])) == distinct, (spacing, max_radius)
            if b_only is not None:
                assert (t2[B & ~A] == b_only).all()


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code) and re.search(r"#define\s+VK_THICK_MAX_REACH\s+32\b", code)
    assert "enum { VK_THICK_CLIP_BOX = 1, VK_THICK_INSTALL = 2 };" in code
    assert re.search(r"int vk_local_thickness\(vk_ctx \*ctx, const vk_thickness_request \*req, const vk_voxel_box \*box, uint32_t \*t2_out, void \*dense_out,\s*"
                     r"vk_thickness_result \*result\);", code)
    assert "static_assert(sizeof(vk_thickness_request) == 36 && sizeof(vk_thickness_result) == 32" in code
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 29\. ", design, flags=re.M)
    section = design[design.index("## 29. "):]
    for phrase in ("T2(v) = max { Dc(u) : u in S, d2(u, v) < Dc(u) }", "C = (uint64_t)floor((double)max_radius * (double)max_radius)", "VK_THICK_INSTALL", "VK_THICK_MAX_REACH"):
        assert phrase in _header(), phrase
        assert phrase in section, phrase
    assert "2^54" in _header()
    for word in ("Loop bounds", "Measurements", "Out of scope"):
        assert word in section, word
    assert "vk_local_thickness" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "local_thickness" in open(os.path.join(ROOT, "README.md")).read() and "--thickness" in open(os.path.join(ROOT, "README.md")).read()
    assert "thick_quick.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "thick_pass_isa.txt"))


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_thick.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(vk_thickness_request), offsetof(vk_thickness_request, flags), '
                   'offsetof(vk_thickness_request, spacing), offsetof(vk_thickness_request, max_radius), offsetof(vk_thickness_request, gain), offsetof(vk_thickness_request, fill_out), '
                   'sizeof(vk_thickness_result), offsetof(vk_thickness_result, sum_t2), offsetof(vk_thickness_result, max_t2), offsetof(vk_thickness_result, gain), '
                   'VK_ABI_VERSION, VK_THICK_MAX_REACH, VK_THICK_INSTALL); return 0; }\n')
    exe = tmp_path / "sizeof_thick"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["36", "8", "12", "24", "28", "32", "32", "16", "24", "28", "5", "32", "2"], out


def test_the_binding_matches_and_every_export_resolves(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert (C.sizeof(N.VkThicknessRequest), C.sizeof(N.VkThicknessResult)) == (36, 32)
    assert [f[0] for f in N.VkThicknessRequest._fields_] == ["lo", "hi", "flags", "spacing", "max_radius", "gain", "fill_out"]
    assert [f[0] for f in N.VkThicknessResult._fields_] == ["n_foreground", "n_saturated", "sum_t2", "max_t2", "gain"]
    assert (N.VkThicknessRequest.spacing.offset, N.VkThicknessRequest.max_radius.offset, N.VkThicknessRequest.fill_out.offset, N.VkThicknessResult.max_t2.offset) == (12, 24, 32, 24)
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert "vk_local_thickness" in declared and declared == set(N.SYMBOLS), declared ^ set(N.SYMBOLS)
    assert hip_built.vk_local_thickness is not None
    # a NULL context: an error, the outputs untouched
    req, res, t2 = N.VkThicknessRequest(), N.VkThicknessResult(7, 7, 7, 7, 7.0), np.full(8, 9, np.uint32)
    assert hip_built.vk_local_thickness(None, C.byref(req), None, t2.ctypes.data, None, C.byref(res)) == -1
    assert (t2 == 9).all() and res.n_foreground == 7 and res.max_t2 == 7


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context
    from vokselis_amd.thickness import Thickness, thickness_request

    assert (V.THICK_MAX_REACH, V.THICK_CLIP_BOX, V.THICK_INSTALL) == (32, 1, 2)
    for name in ("THICK_MAX_REACH", "THICK_CLIP_BOX", "THICK_INSTALL", "VkThicknessRequest", "VkThicknessResult", "Thickness", "thickness_request"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.local_thickness)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("max_radius", 16.0), ("spacing", (1, 1, 1)), ("box", None),
                                                                               ("gain", None), ("fill_out", 0.0), ("install", False), ("out", False), ("t2", False)]
    r = thickness_request(0.3, max_radius=6.5, spacing=(2, 2, 5), gain=0.125, fill_out=0.25, install=True, box="clip")
    assert (r.lo, r.hi, r.flags, list(r.spacing), r.max_radius, r.gain, r.fill_out) == (np.float32(0.3), math.inf, 3, [2, 2, 5], 6.5, 0.125, 0.25)
    r = thickness_request(0.2, 0.4)
    assert (r.flags, list(r.spacing), r.max_radius, r.gain, r.fill_out) == (0, [1, 1, 1], 16.0, 0.0, 0.0)   # gain None: the automatic gain
    for bad in (dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(spacing=(1, 65, 1)), dict(spacing=(1.5, 1, 1)), dict(max_radius=0.5), dict(max_radius=math.nan),
                dict(max_radius=math.inf), dict(gain=0.0), dict(gain=-1.0), dict(gain=math.inf)):
        with pytest.raises(ValueError):
            thickness_request(0.3, **bad)
    t = Thickness(V.VkThicknessResult(10, 3, 250, 36, 0.5))
    assert (t.n_foreground, t.n_saturated, t.sum_t2, t.max_t2, t.gain, t.max_thickness, t.mean_t2, t.t2, t.dense) == (10, 3, 250, 36, 0.5, 12.0, 25.0, None, None)
    assert Thickness(V.VkThicknessResult()).mean_t2 == 0.0


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("thick_fuzz") / "thick_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "thick_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261021"])
def test_validation_order_skips_and_the_replayed_gather_under_sanitizers(fuzz_exe, seed):
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


NEEDS_RANGE = "--thickness needs a value range: --components LO HI, or --iso V for [V, inf)"


@pytest.mark.parametrize("args, message", [
    (["--thickness", "16"], NEEDS_RANGE), (["--thickness", "16", "0.5", "--morph-spacing", "1", "1", "2"], NEEDS_RANGE),
    (["--thickness", "0.5", "--iso", "0.3"], "--thickness MAX_RADIUS [GAIN]: a finite MAX_RADIUS of at least 1"), (["--thickness", "nan", "--iso", "0.3"], "--thickness MAX_RADIUS [GAIN]: a finite MAX_RADIUS of at least 1"),
    (["--thickness", "inf", "--iso", "0.3"], "--thickness MAX_RADIUS [GAIN]: a finite MAX_RADIUS of at least 1"),
    (["--thickness", "33", "--iso", "0.3"], "--thickness MAX_RADIUS [GAIN]: MAX_RADIUS reaches further than 32 voxels of the smallest spacing"),
    (["--thickness", "65", "--morph-spacing", "2", "3", "4", "--iso", "0.3"], "--thickness MAX_RADIUS [GAIN]: MAX_RADIUS reaches further than 32 voxels of the smallest spacing"),
    (["--thickness", "16", "-1", "--iso", "0.3"], "--thickness MAX_RADIUS [GAIN]: a finite GAIN above 0"), (["--thickness", "16", "inf", "--iso", "0.3"], "--thickness MAX_RADIUS [GAIN]: a finite GAIN above 0"),
    (["--thickness"], "missing value for --thickness"),
    (["--iso", "0.3", "--thickness", "16", "--thickness", "8"], "--thickness: at most once"),
    (["--thickness", "16", "--iso", "0.3", "--gpus", "2"], "--thickness runs on one GPU"),
    (["--morph-spacing", "1", "1", "1", "--iso", "0.3"], "--morph-spacing needs --morph"),
])
def test_bonsai_refuses_bad_thickness_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
