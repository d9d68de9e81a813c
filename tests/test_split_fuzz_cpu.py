"""The two references of vk_split_components held together over the shared cases (tests/split_cases.py): the C
restatement (tests/split_restatement.c: breadth-first rounds) and the numpy reference (tests/np_split_reference.py: shortest paths by
relaxation, anchors level by level) -- labels, region table, every total, the cut volume and g itself, bit for bit.  The conditions on the
case list and the figures of the fixed case are asserted, so the list cannot quietly degenerate; the properties of the rule are checked
on every case.  The host side -- the C boundary, vk_split.hpp under ASan + UBSan (tests/split_fuzz.cpp, a stand-alone program), the Python
surface, bonsai's refusals before a device is touched -- needs no GPU either."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import label_cases as LC
import label_helpers as LH
import np_label_reference as NL
import split_cases as SC
import split_helpers as SH

ROOT = LH.ROOT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("split_fuzz_cpu"))


@pytest.fixture(scope="module")
def label_lib(tmp_path_factory):
    return LH.build_restatement(tmp_path_factory.mktemp("split_fuzz_cpu_label"))


@pytest.fixture(scope="module")
def restated(lib):
    return {c.name: SH.restate_case(lib, c) for c in SC.cases()}


def _neighbours_agree(labels, S, conn, test):
    """Whether test(label of v, label of u) holds for every adjacent pair v, u of S, as a count of the pairs where it does not."""
    bad = 0
    for d in NL.offsets(conn):
        (dz, sz), (dy, sy), (dx, sx) = (NL._shifted(labels.shape[a], d[a]) for a in range(3))
        both = S[dz, dy, dx] & S[sz, sy, sx]
        bad += int((both & ~test(labels[dz, dy, dx], labels[sz, sy, sx])).sum())
    return bad


def test_case_list_covers_the_issue(restated):
    cases = SC.cases()
    assert len({c.name for c in cases}) == len(cases) and 40 <= len(cases) <= 80, len(cases)
    assert max(c.vol.size for c in cases) == SC.MAX_VOXELS
    dims = {tuple(reversed(c.vol.shape)) for c in cases}
    assert all(n == 1 or n % t for d in dims for n, t in zip(d, SC.TILE))                       # no dimension is a multiple of the tile
    assert any(1 in d for d in dims) and any(all(n > 2 * t for n, t in zip(d, SC.TILE)) for d in dims)
    assert {c.conn for c in cases} == {6, 18, 26} and {c.kind for c in cases} == {"u8", "u16", "f16"}
    assert any(c.spacing == (1, 1, 2) for c in cases) and any(c.box is not None and c.clip is None for c in cases) and any(c.clip is not None for c in cases)
    res = lambda c: [int(v) for v in restated[c.name][2]]
    # n_regions, n_foreground, n_markers, n_marker_voxels, n_residue_regions, n_residue_voxels, n_cut, rounds
    assert any(res(c)[7] >= 100 for c in cases if "serpentine" in c.name)
    assert any(res(c)[2] and res(c)[4] for c in cases)                                          # unreached regions beside marker regions
    for c in cases:
        r = res(c)
        if "K empty" in c.name:
            assert r[1] > 0 and r[2] == 0 and r[3] == 0 and r[0] == r[4] > 100 and r[7] == 0
        if "S empty" in c.name or "an empty box" in c.name:
            assert r == [0] * 8
        if "S whole" in c.name:
            assert r == [1, c.vol.size, 1, c.vol.size, 0, 0, 0, 0]
        if "percolation at density 0.62" in c.name:
            assert c.radius == 1.0 and r[2] > 100 and r[6] > 1000
        if "specials" in c.name:
            bits = c.vol.view(np.uint16)
            assert ((bits & 0x7fff) > 0x7c00).any() and (bits == 0x7c00).any() and (bits == 0xfc00).any()
    # a tie: a voxel at step k with two neighbours at step k - 1 that carry different anchors
    tie = next(c for c in cases if "a tie" in c.name and c.conn == 6)
    labels, table, result, dense, g = restated[tie.name]
    mid = (4, 4, 18)
    k = int(g[mid])
    assert int(g[4, 4, 17]) == k - 1 == int(g[4, 4, 19]) and labels[4, 4, 17] == 1 and labels[4, 4, 19] == 2 and labels[mid] == 1 and int(result[6]) == 1


def test_the_fixed_case_gives_the_figures_of_the_issue(restated):
    assert int(SC.fixed_mask().sum()) == 4049
    by = {c.radius: restated[c.name] for c in SC.cases() if "fixed" in c.name}
    sizes = lambda r: sorted(int(v) for v in by[r][1][:, 0])
    assert sizes(0.0) == [7, 4042]
    assert [int(v) for v in by[3.0][2][[2, 7, 4, 5]]] == [1, 8, 1, 7] and sizes(3.0) == [7, 4042]
    assert [int(v) for v in by[6.0][2][[2, 7, 4, 5]]] == [2, 11, 1, 7] and sizes(6.0) == [7, 1979, 2063]
    assert [int(v) for v in by[7.5][2][[2, 7, 4, 5]]] == [2, 13, 1, 7] and sizes(7.5) == [7, 1979, 2063]
    labels, table = by[6.0][0], by[6.0][1]
    second = int(labels[10, 11, 22])                                                            # the second ball's centre
    assert int(table[second - 1, 0]) == 1979 and (labels[10, 11, 30:36] == second).all()        # the wire goes to the second
    ndimage = pytest.importorskip("scipy.ndimage")
    S = SC.fixed_mask()
    assert ndimage.label(ndimage.distance_transform_edt(S) ** 2 > 36.0 + 1e-9)[1] == 2


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(restated):
    for c in SC.cases():
        ref = SH.reference_case(c)
        assert LH.differences(restated[c.name][:4], ref[:4]) == "", c.name
        assert (restated[c.name][4] == ref[4]).all(), c.name


def test_properties_of_the_rule(restated, label_lib):
    for c in SC.cases():
        labels, table, result, dense, g = restated[c.name]
        S = NL.foreground(c.vol, c.kind, c.lo, c.hi, c.box)
        n = int(result[0])
        assert len(table) == n and int(table[:, 0].sum()) == int(result[1]) == int(S.sum()) and ((labels != 0) == S).all(), c.name
        assert n == int(result[2]) + int(result[4]), c.name
        if n:
            assert (np.diff(table[:, 1].astype(np.int64)) > 0).all(), c.name                    # ids by increasing anchor
            assert (labels.ravel()[table[:, 1].astype(np.int64)] == np.arange(1, n + 1)).all(), c.name
        # every region is connected: each region is one component of itself
        for k in range(1, n + 1):
            part = labels == k
            assert len(np.unique(NL.first_of_component(part, c.conn)[part])) == 1, (c.name, k)
        # recounts: the markers, the rounds, the cut
        finite = g != 0xFFFFFFFF
        assert int((g == 0).sum()) == int(result[3]) and int(g[finite].max() if finite.any() else 0) == int(result[7]), c.name
        assert int((S & ~finite).sum()) == int(result[5]), c.name
        cut = LH.raw(dense) != LH.raw(c.vol)
        F = LH.raw(NL.fill_bits(c.fill_out, c.kind).reshape(1))[0]
        assert (LH.raw(dense)[cut] == F).all() and not (cut & ~S).any(), c.name
        assert int(cut.sum()) <= int(result[6]), c.name                                         # (a cut voxel whose stored bits are F already does not show)
        # after the cut no two adjacent voxels of S lie in different regions
        left = S & ~_cut_mask(labels, S, c.conn)
        assert int(_cut_mask(labels, S, c.conn).sum()) == int(result[6]), c.name
        assert _neighbours_agree(labels, left, c.conn, lambda a, b: a == b) == 0, c.name
        # label_components of the cut volume never joins two regions
        lab2 = LH.restate(label_lib, dense, c.kind, c.lo, c.hi, c.conn, c.box)[0]
        pairs = np.unique(np.stack([lab2[lab2 != 0].astype(np.int64), labels[lab2 != 0].astype(np.int64)]), axis=1)
        assert len(np.unique(pairs[0])) == pairs.shape[1], c.name
        # radius 0, or a radius that leaves K empty: the label restatement's output
        if c.radius == 0.0 or int(result[3]) == 0:
            ref = LH.restate(label_lib, c.vol, c.kind, c.lo, c.hi, c.conn, c.box)
            assert (ref[0] == labels).all() and (ref[1] == table).all() and int(result[6]) == 0, c.name


def _cut_mask(labels, S, conn):
    big = np.int64(1) << 40
    ids = np.where(S, labels.astype(np.int64), big)
    m = np.full(ids.shape, big)
    for d in NL.offsets(conn):
        (dz, sz), (dy, sy), (dx, sx) = (NL._shifted(ids.shape[a], d[a]) for a in range(3))
        m[dz, dy, dx] = np.minimum(m[dz, dy, dx], ids[sz, sy, sx])
    return S & (m < ids)


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert "enum { VK_SPLIT_CLIP_BOX = 1, VK_SPLIT_INSTALL = 2 };" in code
    assert re.search(r"int vk_split_components\(vk_ctx \*ctx, const vk_split_request \*req, const vk_voxel_box \*box, uint32_t \*labels_out, vk_component \*components,\s*"
                     r"uint64_t cap_components, void \*dense_out, vk_split_result \*result\);", code)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 27\. ", design, flags=re.M)
    section = design[design.index("## 27. "):]
    for phrase in ("D2(not S, v) > R2", "x + nx (y + ny z)", "g(u) = k - 1", "VK_SPLIT_INSTALL"):
        assert phrase in _header(), phrase
        assert phrase in section, phrase
    for word in ("Visibility", "Termination"):
        assert word in section, word
    assert "vk_split_components" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "split_pass_isa.txt"))


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_split.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(vk_split_request), offsetof(vk_split_request, connectivity), '
                   'offsetof(vk_split_request, spacing), offsetof(vk_split_request, radius), offsetof(vk_split_request, fill_out), offsetof(vk_split_request, pad), '
                   'sizeof(vk_split_result), offsetof(vk_split_result, n_cut), offsetof(vk_split_result, rounds), VK_ABI_VERSION, VK_SPLIT_CLIP_BOX, VK_SPLIT_INSTALL); return 0; }\n')
    exe = tmp_path / "sizeof_split"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["40", "8", "16", "28", "32", "36", "64", "48", "56", "5", "1", "2"], out


def test_the_binding_matches_and_every_export_resolves(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert (C.sizeof(N.VkSplitRequest), C.sizeof(N.VkSplitResult)) == (40, 64)
    assert [f[0] for f in N.VkSplitRequest._fields_] == ["lo", "hi", "connectivity", "flags", "spacing", "radius", "fill_out", "pad"]
    assert [f[0] for f in N.VkSplitResult._fields_] == list(SH.RESULT_FIELDS) + ["pad"]
    assert (N.VkSplitRequest.spacing.offset, N.VkSplitRequest.radius.offset, N.VkSplitResult.rounds.offset) == (16, 28, 56)
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert "vk_split_components" in declared and declared == set(N.SYMBOLS), declared ^ set(N.SYMBOLS)
    assert hip_built.vk_split_components is not None
    # a NULL context: an error, the outputs untouched
    req, res, lab = N.VkSplitRequest(), N.VkSplitResult(), np.full(8, 9, np.uint32)
    res.n_regions = 7
    assert hip_built.vk_split_components(None, C.byref(req), None, lab.ctypes.data, None, 0, None, C.byref(res)) == -1
    assert (lab == 9).all() and res.n_regions == 7


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context

    assert (V.SPLIT_CLIP_BOX, V.SPLIT_INSTALL) == (1, 2)
    for name in ("SPLIT_CLIP_BOX", "SPLIT_INSTALL", "VkSplitRequest", "VkSplitResult", "Regions", "split_request"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.split_components)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("radius", 0.0), ("spacing", (1, 1, 1)), ("connectivity", 6),
                                                                                 ("box", None), ("labels", False), ("fill_out", 0.0), ("install", False), ("out", False)]
    r = V.split_request(0.3, radius=2.5, spacing=(1, 2, 3), connectivity=26, box="clip", fill_out=0.1, install=True)
    assert (r.lo, r.hi, r.connectivity, r.flags, list(r.spacing), r.radius, r.fill_out, r.pad) == (np.float32(0.3), math.inf, 26, 3, [1, 2, 3], 2.5, np.float32(0.1), 0)
    for bad in (dict(radius=-1.0), dict(radius=math.nan), dict(radius=1e9), dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(spacing=(1, 1.5, 1)), dict(spacing=(1, 1, 65))):
        with pytest.raises(ValueError):
            V.split_request(0.3, **bad)
    table = (V.VkComponent * 2)()
    table[0].n_voxels, table[1].n_voxels = 5, 9
    res = V.VkSplitResult()
    res.n_regions, res.n_foreground, res.n_markers, res.n_residue_regions, res.n_cut, res.rounds = 2, 14, 1, 1, 3, 4
    regions = V.Regions(table, res)
    assert regions.n == 2 and list(regions.largest(1)) == [2] and (regions.n_markers, regions.n_residue_regions, regions.n_cut, regions.rounds) == (1, 1, 3, 4) and regions.labels is None


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split_fuzz") / "split_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "split_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261020"])
def test_validation_tiles_seams_from_an_array_and_the_growth_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "200", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (200 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.fixture(scope="module")
def bonsai():
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(ROOT, "vokselis_amd", "_lib", "bonsai")
    assert os.path.exists(exe)
    return exe


@pytest.mark.parametrize("args, message", [
    (["--split", "3"], "--split needs a value range: --components LO HI, or --iso V for [V, inf)"),
    (["--split", "nan", "--iso", "0.3"], "--split RADIUS [CONN]: a finite RADIUS of 0 .. 65535"),
    (["--split", "inf", "--iso", "0.3"], "--split RADIUS [CONN]: a finite RADIUS of 0 .. 65535"),
    (["--split", "-1", "--components", "0.3", "inf"], "--split RADIUS [CONN]: a finite RADIUS of 0 .. 65535"),
    (["--split", "70000", "--iso", "0.3"], "--split RADIUS [CONN]: a finite RADIUS of 0 .. 65535"),
    (["--split", "2", "8", "--iso", "0.3"], "--split RADIUS [CONN]: CONN is 6, 18 or 26"),
    (["--split"], "missing value for --split"),
    (["--split", "2", "--iso", "0.3", "--gpus", "2"], "--split runs on one GPU"),
    (["--split", "2", "--iso", "0.3", "--label-fill", "nan"], "--label-fill V: V must be finite"),
    (["--split", "2", "--iso", "0.3", "--morph-fill", "1", "0"], "--morph-fill needs --morph"),
    (["--split", "2", "--iso", "0.3", "--morph-spacing", "0", "1", "1"], "--morph-spacing SX SY SZ: integers of 1 .. 64"),
])
def test_bonsai_refuses_bad_split_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
