"""The two references of vk_label_components held together over the shared cases (tests/label_cases.py): the C
restatement (tests/label_restatement.c: a raster scan with a flood fill) and the numpy reference (tests/np_label_reference.py: minimum
labels propagated until nothing changes) -- labels, component table, totals and masked volume, bit for bit; both against
scipy.ndimage.label where scipy imports.  The conditions on the case list are asserted, so the list cannot quietly degenerate.  The host
side -- the C boundary, vk_label.hpp under ASan + UBSan (tests/label_fuzz.cpp, a stand-alone program), the Python surface -- needs no GPU
either."""
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

ROOT = LH.ROOT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return LH.build_restatement(tmp_path_factory.mktemp("label_fuzz_cpu"))


@pytest.fixture(scope="module")
def restated(lib):
    return {c.name: LH.restate_case(lib, c) for c in LC.cases()}


def _tile_in_the_header():
    src = open(os.path.join(ROOT, "vokselis_amd", "csrc", "vk_label.hpp")).read()
    return tuple(int(v) for v in re.findall(r"(\d+)u", re.search(r"kLabelTile = \{(.*?)\};", src).group(1)))[:3]


def test_case_list_covers_the_issue(restated):
    cases = LC.cases()
    assert len({c.name for c in cases}) == len(cases) and 150 <= len(cases) <= 400, len(cases)
    assert max(c.vol.size for c in cases) <= LC.MAX_VOXELS
    assert _tile_in_the_header() == LC.TILE
    dims = {tuple(reversed(c.vol.shape)) for c in cases}
    assert dims == set(LC.DIMS) and {(1, 1, 1), (70, 1, 1), (1, 1, 70), (37, 21, 11), (48, 40, 33)} <= dims
    assert all(n == 1 or n % t for d in dims for n, t in zip(d, LC.TILE))          # no dimension is a multiple of the tile
    assert all(any(d[a] > 2 * LC.TILE[a] for d in dims) for a in range(3))         # more than two tiles along every axis
    for kind in ("u8", "u16", "f16"):
        mine = [c for c in cases if c.kind == kind]
        text = " | ".join(c.name for c in mine)
        for word in ("uniform noise", "percolation", "all foreground", "all background", "checkerboard", "along an edge", "at a corner", "serpentine", "spiral", "U joined", "empty box",
                     "one voxel thick", "cuts components", "clip box", "largest 1", "ties in size", "above n", "min size 1", "above the largest", "seeds: background", "INVERT"):
            assert word in text, (kind, word)
        assert {c.conn for c in mine} == {6, 18, 26} and {c.keep for c in mine} == {"all", "largest", "min_size", "seeds"}
        assert any(c.lo == c.hi for c in mine) and any(c.lo == -math.inf for c in mine) and any(c.hi == math.inf for c in mine)
        for keep in ("largest", "min_size", "seeds"):
            assert {c.invert for c in mine if c.keep == keep} == {False, True}, (kind, keep)
    special = [c for c in cases if "NaN, inf" in c.name]
    assert {(c.lo, c.hi) for c in special} >= {(-math.inf, math.inf), (math.inf, math.inf), (-math.inf, -math.inf), (0.0, 0.0)}
    # what the cases exercise, on the restatement's output
    by = {c.name: c for c in cases}
    n_of = lambda name: int(restated[name][2][0])
    for kind in ("u8", "u16", "f16"):
        cb = f"{kind} (35, 10, 9) checkerboard, [1.0, 1.0] conn %d, keep all"
        assert n_of(cb % 6) == (35 * 10 * 9 + 1) // 2 and n_of(cb % 18) == 1 and n_of(cb % 26) == 1        # every voxel its own component at 6
        edge = f"{kind} (37, 21, 11) two blocks touching along an edge, [1.0, 1.0] conn %d, keep all"
        assert (n_of(edge % 6), n_of(edge % 18), n_of(edge % 26)) == (2, 1, 1)
        corner = f"{kind} (37, 21, 11) two blocks touching at a corner, [1.0, 1.0] conn %d, keep all"
        assert (n_of(corner % 6), n_of(corner % 18), n_of(corner % 26)) == (2, 2, 1)
        for word, least in (("serpentine", 800), ("spiral", 1500), ("U joined", 80)):
            c = next(c for c in cases if c.kind == kind and word in c.name and c.conn == 6 and c.keep == "all")
            labels, table, result, _ = restated[c.name]
            assert int(result[0]) == 1 and int(result[1]) >= least, (c.name, result)                           # one long chain
        assert n_of(f"{kind} (37, 21, 11) constant, all foreground, [0.5, inf] conn 6, largest 1") == 1
        assert n_of(f"{kind} (37, 21, 11) constant, all background, [0.5, inf] conn 6, largest 1") == 0
        perc = restated[f"{kind} (48, 40, 33) percolation at density 0.31, [0.5, inf] conn 6, keep all"]
        sizes = perc[1][:, 0]
        assert len(sizes) > 1000 and sizes.max() > 500 and (sizes == 1).sum() > 100                           # components of every size
        boxes = perc[1][:, 2:]
        big = boxes[int(np.argmax(sizes))].astype(np.int64)
        assert all((big[3 + a] - 1) // LC.TILE[a] != big[a] // LC.TILE[a] for a in range(3))                  # ... across seams on every axis
        assert ((boxes[:, 3:] - 1) // np.array(LC.TILE) != boxes[:, :3] // np.array(LC.TILE)).any(axis=1).sum() > 100  # and many small ones across one
        ties = restated[next(c.name for c in cases if c.kind == kind and "percolation" in c.name and "largest 3, ties" in c.name and not c.invert)]
        assert int(ties[2][2]) == 3
        seeds = next(c for c in cases if c.kind == kind and "percolation" in c.name and "seeds: background" in c.name and not c.invert)
        assert len(seeds.seeds) == 4 and int(restated[seeds.name][2][2]) == 1                                 # two seeds in one component, one on background, one outside the box
        empty = restated[next(c.name for c in cases if c.kind == kind and "percolation" in c.name and "empty box" in c.name)]
        assert int(empty[2][0]) == 0 and not empty[0].any()
    assert by  # (the names above exist: a KeyError otherwise)


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(restated):
    for c in LC.cases():
        assert LH.differences(restated[c.name], LH.reference_case(c)) == "", c.name


def test_both_agree_with_scipy_after_renumbering_by_first_voxel(restated):
    ndimage = pytest.importorskip("scipy.ndimage")
    done = set()
    for c in LC.cases():
        key = (c.vol_id, c.lo, c.hi, c.conn, c.box)
        if key in done:
            continue
        done.add(key)
        fg = NL.foreground(c.vol, c.kind, c.lo, c.hi, c.box)
        lab, n = ndimage.label(fg, structure=ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[c.conn]))
        want = NL.renumber_by_first(lab)
        assert n == int(restated[c.name][2][0]) and (want == restated[c.name][0]).all(), c.name
        assert (want == NL.label(c.vol, c.kind, c.lo, c.hi, c.conn, c.box)[0]).all(), c.name
    assert len(done) > 60


def test_properties_of_the_rule(restated):
    for c in LC.cases():
        labels, table, result, dense = restated[c.name]
        n = int(result[0])
        assert len(table) == n and int(table[:, 0].sum()) == int(result[1]) == int((labels != 0).sum()), c.name
        flat = labels.ravel()
        if n:
            assert (np.diff(table[:, 1].astype(np.int64)) > 0).all(), c.name                                  # ids by increasing first
            assert (flat[table[:, 1].astype(np.int64)] == np.arange(1, n + 1)).all(), c.name                  # first carries its own id ...
            first_seen = np.array([np.flatnonzero(flat == k)[0] for k in range(1, min(n, 20) + 1)])
            assert (first_seen == table[:len(first_seen), 1].astype(np.int64)).all(), c.name                  # ... and is the first voxel with it
        kept = dense.view(np.uint16) if dense.dtype == np.float16 else dense
        orig = LH.raw(c.vol)
        F = LH.raw(NL.fill_bits(c.fill, c.kind).reshape(1))[0]
        assert ((kept == orig) | (kept == F)).all(), c.name                                                   # a voxel keeps its bits or becomes F
        if c.keep == "all":
            assert ((kept == orig) | ((labels == 0) != c.invert)).all(), c.name


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code) and re.search(r"#define\s+VK_LABEL_MAX_SEEDS\s+16\b", code)
    assert "enum { VK_LABEL_KEEP_ALL = 0, VK_LABEL_KEEP_LARGEST = 1, VK_LABEL_KEEP_MIN_SIZE = 2, VK_LABEL_KEEP_SEEDS = 3 };" in code
    assert "enum { VK_LABEL_CLIP_BOX = 1, VK_LABEL_INSTALL = 2, VK_LABEL_INVERT = 4 };" in code
    assert re.search(r"int vk_label_components\(vk_ctx \*ctx, const vk_label_request \*req, const vk_voxel_box \*box, uint32_t \*labels_out, vk_component \*components,\s*"
                     r"uint64_t cap_components, void \*dense_out, vk_label_result \*result\);", code)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 24\. ", design, flags=re.M)
    section = design[design.index("## 24. "):]
    for phrase in ("t >= lo_k && t <= hi_k", "sum |d_c| <= 1", "x + nx (y + ny z)", "n_voxels descending, then first ascending", "VK_LABEL_INVERT", "VK_LABEL_INSTALL"):
        assert phrase in _header(), phrase
        assert phrase in section, phrase
    for word in ("Visibility", "Termination", "32 x 16 x 8"):
        assert word in section, word
    assert "vk_label_components" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "label_pass_isa.txt"))


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_label.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(vk_label_request), offsetof(vk_label_request, connectivity), '
                   'offsetof(vk_label_request, keep), offsetof(vk_label_request, count), offsetof(vk_label_request, fill), offsetof(vk_label_request, seeds), '
                   'sizeof(vk_component), offsetof(vk_component, box), sizeof(vk_label_result), offsetof(vk_label_result, n_kept_voxels), '
                   'VK_ABI_VERSION, VK_LABEL_MAX_SEEDS, VK_LABEL_KEEP_SEEDS, VK_LABEL_INSTALL, VK_LABEL_INVERT); return 0; }\n')
    exe = tmp_path / "sizeof_label"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["232", "8", "16", "24", "32", "40", "40", "16", "32", "24", "5", "16", "3", "2", "4"], out


def test_the_binding_matches_and_every_export_resolves(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert (C.sizeof(N.VkLabelRequest), C.sizeof(N.VkComponent), C.sizeof(N.VkLabelResult)) == (232, 40, 32)
    assert [f[0] for f in N.VkLabelRequest._fields_] == ["lo", "hi", "connectivity", "flags", "keep", "n_seeds", "count", "fill", "pad", "seeds"]
    assert (N.VkLabelRequest.count.offset, N.VkLabelRequest.fill.offset, N.VkLabelRequest.seeds.offset, N.VkComponent.box.offset) == (24, 32, 40, 16)
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert "vk_label_components" in declared and declared == set(N.SYMBOLS), declared ^ set(N.SYMBOLS)
    for name in N.SYMBOLS:
        assert getattr(hip_built, name) is not None, name
    # a NULL context: an error, the outputs untouched
    req, res, lab = N.VkLabelRequest(), N.VkLabelResult(7, 7, 7, 7), np.full(8, 9, np.uint32)
    assert hip_built.vk_label_components(None, C.byref(req), None, lab.ctypes.data, None, 0, None, C.byref(res)) == -1
    assert (lab == 9).all() and res.n_components == 7


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context
    from vokselis_amd.label import label_request

    assert (V.LABEL_MAX_SEEDS, V.LABEL_KEEP_ALL, V.LABEL_KEEP_LARGEST, V.LABEL_KEEP_MIN_SIZE, V.LABEL_KEEP_SEEDS, V.LABEL_CLIP_BOX, V.LABEL_INSTALL, V.LABEL_INVERT) == (16, 0, 1, 2, 3, 1, 2, 4)
    for name in ("LABEL_MAX_SEEDS", "LABEL_KEEP_SEEDS", "LABEL_INVERT", "VkLabelRequest", "VkComponent", "VkLabelResult", "Components", "voxel_of"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.label_components)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("connectivity", 6), ("box", None), ("labels", False)]
    sig = inspect.signature(Context.keep_components)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("keep", "largest"), ("count", 1), ("seeds", ()), ("invert", False),
                                                                                ("fill", 0.0), ("connectivity", 6), ("box", None), ("install", True), ("out", False)]
    r = label_request(0.3, keep="seeds", seeds=[(1, 2, 3), (4, 5, 6)], invert=True, install=True, box="clip", fill=0.5, connectivity=26)
    assert (r.lo, r.hi, r.connectivity, r.flags, r.keep, r.n_seeds, r.count, r.fill, r.pad) == (np.float32(0.3), math.inf, 26, 7, 3, 2, 0, 0.5, 0)
    assert list(r.seeds[1]) == [4, 5, 6] and list(r.seeds[2]) == [0, 0, 0]
    assert label_request(0.1, 0.2, keep="largest", count=5).count == 5 and label_request(0.1, keep="min_size", count=9).keep == 2 and label_request(0.1).count == 0
    for bad in (dict(keep="biggest"), dict(keep="seeds", seeds=[(1, 2)]), dict(keep="seeds", seeds=[(0, 0, 0)] * 17), dict(keep="seeds", seeds=[(0, -1, 0)]), dict(keep="largest", count=-1), dict(keep="largest", count=0), dict(keep="min_size", count=0)):
        with pytest.raises(ValueError):
            label_request(0.3, **bad)
    # voxel_of: min(floor(pos n), n - 1)
    assert V.voxel_of((0.0, 0.5, 1.0), (10, 9, 8)) == (0, 4, 7) and V.voxel_of((0.999, 0.1, 0.25), (3, 10, 4)) == (2, 1, 1)
    for x in range(7):
        assert V.voxel_of(((x + 0.5) / 7, 0.0, 0.0), (7, 1, 1))[0] == x                                       # a texel's centre lies in its voxel
    for bad in ((1.5, 0, 0), (-0.1, 0, 0), (math.nan, 0, 0)):
        with pytest.raises(ValueError):
            V.voxel_of(bad, (4, 4, 4))
    table = (V.VkComponent * 3)()
    for k, (size, first) in enumerate(((5, 0), (9, 3), (9, 7))):
        table[k].n_voxels, table[k].first = size, first
    comps = V.Components(table, 3, 23)
    assert comps.n == 3 and list(comps.sizes) == [5, 9, 9] and list(comps.largest(2)) == [2, 3] and list(comps.largest(9)) == [2, 3, 1] and comps.boxes.shape == (3, 6)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("label_fuzz") / "label_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "label_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261020"])
def test_union_find_tiles_seams_scan_and_selection_under_sanitizers(fuzz_exe, seed):
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


NEEDS_RANGE = "need a value range: --components LO HI, or --iso V for [V, inf)"


@pytest.mark.parametrize("args, message", [
    (["--keep-largest", "1"], NEEDS_RANGE), (["--drop-islands", "5"], NEEDS_RANGE), (["--keep-voxel", "1", "2", "3"], NEEDS_RANGE), (["--remove-voxel", "1", "2", "3"], NEEDS_RANGE),
    (["--keep-pick", "3", "3", "--components", "0.3", "inf"], "--keep-pick needs --iso"),
    (["--label-fill", "0.5", "--components", "0.3", "inf"], "--label-fill needs a flag that drops voxels"),
    (["--label-fill", "nan", "--iso", "0.3", "--keep-largest", "1"], "--label-fill V: V must be finite"),
    (["--components", "0.5", "0.3"], "needs LO <= HI"), (["--components", "nan", "1"], "needs LO <= HI"), (["--components", "0.1", "0.2", "8"], "CONN is 6, 18 or 26"),
    (["--components", "0.1"], "missing value for --components"), (["--keep-voxel", "1", "2"], "missing value for --keep-voxel"),
    (["--keep-largest", "0", "--iso", "0.3"], "--keep-largest: a count of at least 1"), (["--drop-islands", "-2", "--iso", "0.3"], "--drop-islands: a count of at least 1"),
    (["--remove-voxel", "1", "-2", "3", "--iso", "0.3"], "--remove-voxel X Y Z: voxel indices >= 0"),
    (["--iso", "0.3"] + ["--keep-largest", "1"] * 17, "--keep-largest: at most 16 times"), (["--iso", "0.3"] + ["--keep-voxel", "1", "1", "1"] * 17, "--keep-voxel: at most 16 times"),
    (["--iso", "0.3"] + ["--keep-voxel", "1", "1", "1"] * 9 + ["--keep-pick", "1", "1"] * 8, "at most 16 seeds together"),
    (["--components", "0.3", "inf", "--gpus", "2"], "--components and the keep flags run on one GPU"),
    (["--save-raw", "out.raw", "--components", "0.3", "inf"], "--save-raw writes the filtered volume: it needs --median or --smooth"),
])
def test_bonsai_refuses_bad_component_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
