"""The two references of vk_skeletonize held together over the shared cases (tests/skel_cases.py): the C
restatement (tests/skel_restatement.c: sequential, a flood fill over explicit 3 x 3 x 3 arrays) and the numpy reference
(tests/np_skel_reference.py: whole arrays, shifted views, a table over the masks that occur) -- classes, dense array and totals, bit for
bit; the fixed cases with their pinned counts; the invariants of a topology-preserving thinning on every case.  The conditions on the
case list are asserted on the restatement's output, so the list cannot quietly degenerate.  The host side -- the C boundary, vk_skel.hpp
under ASan + UBSan and over all 2^26 masks (tests/skel_fuzz.cpp, a stand-alone program), the Python surface, bonsai's argument handling
-- needs no GPU either."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dist_cases as DC
import np_label_reference as NL
import np_skel_reference as NS
import skel_cases as SC
import skel_helpers as SH

ROOT = SH.ROOT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return SH.build_restatement(tmp_path_factory.mktemp("skel_fuzz_cpu"))


@pytest.fixture(scope="module")
def restated(lib):
    return {c.name: SH.restate_case(lib, c) for c in SC.cases()}


@pytest.fixture(scope="module")
def referenced():
    return {c.name: SH.reference_case(c) for c in SC.cases()}


def _dims(c):
    return tuple(reversed(c.vol.shape))


def _set(c):
    return NL.foreground(np.asarray(c.vol), c.kind, c.lo, c.hi, c.box)


def test_case_list_covers_the_issue(restated, lib):
    cases = SC.cases()
    assert len({c.name for c in cases}) == len(cases) and 100 <= len(cases) <= 200, len(cases)
    assert max(c.vol.size for c in cases) <= SC.MAX_VOXELS
    src = open(os.path.join(ROOT, "vokselis_amd", "csrc", "vk_label.hpp")).read()
    assert tuple(int(v) for v in re.search(r"kLabelTile = \{(\d+)u, (\d+)u, (\d+)u,", src).groups()) == SC.TILE == (32, 16, 8)
    dims = {_dims(c) for c in cases}
    assert set(SC.DIMS) | {SC.BIG, SC.SHAPES, SC.LINE, (37, 21, 11), (26, 5, 5), (12, 7, 3)} <= dims
    assert all(any(d[a] == 1 and max(d) > 1 for d in dims) for a in range(3))                                   # 1 on each axis in turn
    assert any(all(n % t for n, t in zip(d, SC.TILE)) for d in dims) and any(all(n % t == 0 for n, t in zip(d, SC.TILE)) for d in dims)
    assert all(n > 2 * t for n, t in zip(SC.BIG, SC.TILE))                                                      # 3 x 3 x 3 tiles
    assert all(v % 2 == 1 for v in SC.ODD_BOX[:3])                                                              # absolute and box-relative parity differ on every axis
    by = {c.name: (c, restated[c.name]) for c in cases}
    for kind in ("u8", "u16", "f16"):
        mine = [c for c in cases if c.kind == kind]
        text = " | ".join(c.name for c in mine)
        for word in ("empty,", "full,", "a bar", "a plate", "a ball", "a ring", "a hollow shell", "a tube-wall torus", "the fixed bar", "the fixed slabs", "a line through five tiles",
                     "density 0.31", "density 0.6", "density 0.9", ", box (", "clip box", "empty box", "uniform noise", "stopped early"):
            assert word in text, (kind, word)
        assert {c.mode for c in mine} == {SC.CURVE, SC.KERNEL} and {c.fill_in is None for c in mine} == {True, False}
        assert any(c.box == SC.ODD_BOX for c in mine)
        clipped = [c for c in mine if c.clip is not None]
        assert clipped and all(v % 2 == 1 for c in clipped for v in c.box[:3]), [c.box for c in clipped]
        assert any(c.box is not None and c.box[0] == c.box[3] for c in mine)                                    # an empty box
    special = [c for c in cases if "NaN, inf" in c.name]
    assert {(c.lo, c.hi) for c in special} >= {(-math.inf, math.inf), (0.0, math.inf), (-math.inf, 0.0), (math.inf, math.inf), (-math.inf, -math.inf)}
    assert all(int(by[c.name][1][2][0]) > 0 for c in special)

    # what the cases exercise, on the restatement's output: result = n_foreground, n_skeleton, n_isolated, n_end, n_regular, n_junction, links[13], iterations, converged
    def one(word, kind="u8", **where):
        return next((c, r) for c, r in by.values() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))

    c, r = one("empty,")
    assert not r[2][:20].any() and int(r[2][20]) == 1 and not r[0].any()                                        # the empty set: nothing, converged at once
    c, r = one("full,", mode=SC.KERNEL)
    assert int(r[2][0]) == c.vol.size and [int(v) for v in r[2][1:6]] == [1, 1, 0, 0, 0]                        # a full block's kernel: one voxel
    c, r = one("empty box")
    assert not r[2][:20].any() and c.box[0] == c.box[3]
    # each shape straddles the tile corner: it has voxels in all eight tiles around (32, 16, 8); and its topology is what its name says
    numbers = {"a bar": (1, 1, 1), "a plate": (1, 1, 1), "a ball": (1, 1, 1), "a ring": (1, 1, 0), "a hollow shell": (1, 2, 2), "a tube-wall torus": (1, 2, 0)}
    for word, topo in numbers.items():
        c, r = one(word + " on the tile corner", max_iterations=0)
        s = _set(c)
        z, y, x = np.nonzero(s)
        assert len({(int(a) >= SC.CORNER[0], int(b) >= SC.CORNER[1], int(d) >= SC.CORNER[2]) for a, b, d in zip(x, y, z)}) == 8, word
        assert SH.topology(s) == topo, (word, SH.topology(s))
    c, r = one("a ring", mode=SC.KERNEL)
    assert int(r[2][1]) == int(r[2][4]) > 20 and int(r[2][3]) == 0                                              # a ring's kernel: a closed curve, every voxel regular
    c, r = one("a hollow shell", mode=SC.KERNEL)
    assert SH.topology(r[0] != 0) == (1, 2, 2) and int(r[2][1]) > 100                                           # a shell stays a closed surface
    c, r = one("a tube-wall torus", mode=SC.KERNEL)
    assert SH.topology(r[0] != 0) == (1, 2, 0)                                                                  # two tunnels: Euler characteristic 0 with a cavity
    # a structure at least 7 voxels thick that needs at least 3 iterations
    c, r = one("a ball on the tile corner", mode=SC.KERNEL, max_iterations=0)
    s = _set(c)
    assert min(int(s.any(axis=tuple(a for a in range(3) if a != ax)).sum()) for ax in range(3)) >= 7 and int(r[2][19]) >= 3 and int(r[2][1]) == 1
    # stopped by max_iterations
    stopped = [(c, r) for c, r in by.values() if c.max_iterations]
    assert len(stopped) >= 6 and all(int(r[2][20]) == 0 and int(r[2][19]) == c.max_iterations for c, r in stopped)
    assert all(int(r[2][20]) == 1 for c, r in by.values() if not c.max_iterations)
    # a tile that sleeps for an iteration and is woken by a neighbour's deletion: the middle tile of the line
    c, r = one("a line through five tiles")
    deleted, active = SH.tile_activity(SH.snapshots(lib, c))
    middle = [bool(a[0, 0, 2]) for a in active]
    assert middle[0] and not middle[1] and any(middle[2:]), middle
    woken = middle.index(True, 2)
    assert not deleted[woken - 1][0, 0, 2] and (deleted[woken - 1][0, 0, 1] or deleted[woken - 1][0, 0, 3]) and any(bool(d[0, 0, 2]) for d in deleted[woken:])
    assert int(r[2][19]) == len(deleted) >= 30
    # all five classes in one case; all 13 link directions in one case
    assert any(set(np.unique(r[0]).tolist()) == {0, 1, 2, 3, 4} for _, r in by.values())
    assert any((r[2][SH.R_LINKS:SH.R_LINKS + 13] > 0).all() for _, r in by.values())
    assert sum(int(r[2][19]) >= 5 for _, r in by.values()) > 20


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(restated, referenced):
    for c in SC.cases():
        assert SH.differences(restated[c.name], referenced[c.name]) == "", c.name


def test_the_fixed_cases_give_the_pinned_counts(lib):
    # n_foreground, n_skeleton, n_isolated, n_end, n_regular, n_junction, iterations, converged
    bar = DC.mask_volume(SC.fixed_bar(), "u8")
    slabs = DC.mask_volume(SC.fixed_slabs(), "u8")
    assert int(SC.fixed_slabs().sum()) == 206
    pinned = ((bar, SC.CURVE, (650, 26, 0, 5, 20, 1, 2, 1)), (bar, SC.KERNEL, None), (slabs, SC.KERNEL, (206, 18, 0, 0, 9, 9, 5, 1)))
    for vol, mode, want in pinned:
        for got in (SH.restate(lib, vol, "u8", 0.5, math.inf, mode), NS.apply(vol, "u8", 0.5, math.inf, mode, 0, None, 0.0, None)):
            r = [int(v) for v in got[2]]
            if want is None:  # the bar's kernel: one voxel
                assert r[:6] == [650, 1, 1, 0, 0, 0] and r[20] == 1
                continue
            assert tuple(r[:6] + r[19:21]) == want, (mode, r)
    # the bar in curve mode: the centre line along x plus four one-voxel corner spurs at one end
    cls = SH.restate(lib, bar, "u8", 0.5, math.inf, SC.CURVE)[0]
    z, y, x = np.nonzero(cls)
    line = (y == 2) & (z == 2)
    assert int(line.sum()) == 22 and len(set(x[~line].tolist())) == 1 and sorted(zip(y[~line].tolist(), z[~line].tolist())) == [(1, 1), (1, 3), (3, 1), (3, 3)]


def test_thinning_preserves_the_topology_on_every_case(lib, restated, referenced):
    face_bits = np.uint32(sum(1 << int(b) for b in NS._FACES))
    for c in SC.cases():
        s = _set(c)
        for got in (restated[c.name], referenced[c.name]):
            k = got[0] != 0
            assert not (k & ~s).any(), c.name                                                                   # never a voxel added
            assert int(got[2][0]) == int(s.sum()) and int(got[2][1]) == int(k.sum())
        k = restated[c.name][0] != 0
        assert (k == (referenced[c.name][0] != 0)).all()
        assert SH.topology(k) == SH.topology(s), (c.name, SH.topology(s), SH.topology(k))                       # 26-components, 6-components of the padded background, Euler characteristic
        if not int(restated[c.name][2][SH.R_CONVERGED]):
            continue
        again = SH.restate(lib, DC.mask_volume(k, "u8"), "u8", 0.5, math.inf, c.mode)                           # thinning K again returns K
        assert ((again[0] != 0) == k).all() and int(again[2][SH.R_ITERATIONS]) == 0, c.name
        if c.mode == SC.KERNEL:                                                                                 # no voxel of a converged kernel is a simple candidate
            m = NS.masks(k)
            cand = k & ((m & face_bits) != face_bits)
            assert not any(NS.simple(v) for v in np.unique(m[cand])), c.name


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert "enum { VK_SKEL_CURVE = 0, VK_SKEL_KERNEL = 1 };" in code and "enum { VK_SKEL_CLIP_BOX = 1, VK_SKEL_INSTALL = 2, VK_SKEL_FILL_IN = 4 };" in code
    assert "enum { VK_SKEL_OFF = 0, VK_SKEL_ISOLATED = 1, VK_SKEL_END = 2, VK_SKEL_REGULAR = 3, VK_SKEL_JUNCTION = 4 };" in code
    assert re.search(r"int vk_skeletonize\(vk_ctx \*ctx, const vk_skeleton_request \*req, const vk_voxel_box \*box, uint8_t \*class_out, void \*dense_out,\s*vk_skeleton_result \*result\);", code)
    assert "static_assert(sizeof(vk_skeleton_request) == 32 && sizeof(vk_skeleton_result) == 160" in code
    assert "_Static_assert(sizeof(vk_skeleton_request) == 32 && sizeof(vk_skeleton_result) == 160" in code
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 31\. ", design, flags=re.M)
    section = design[design.index("## 31. "):]
    for phrase in ("Malandain and Bertrand", "VK_SKEL_INSTALL", "sf(v) = (x & 1) | (y & 1) << 1 | (z & 1) << 2"):
        assert phrase in _header(), phrase
        assert phrase in section, phrase
    for word in ("The rule", "Structure", "Why the result depends on no order", "Loop bounds and barriers", "Resources", "Measurements", "Checks", "Out of scope"):
        assert word in section, word
    assert "vk_skeletonize" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "skeletonize" in open(os.path.join(ROOT, "README.md")).read() and "--skeleton" in open(os.path.join(ROOT, "README.md")).read()
    assert "skel_quick.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "skel_pass_isa.txt"))


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_skel.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(vk_skeleton_request), offsetof(vk_skeleton_request, mode), '
                   'offsetof(vk_skeleton_request, flags), offsetof(vk_skeleton_request, max_iterations), offsetof(vk_skeleton_request, fill_in), offsetof(vk_skeleton_request, fill_out), '
                   'offsetof(vk_skeleton_request, pad), sizeof(vk_skeleton_result), offsetof(vk_skeleton_result, links), offsetof(vk_skeleton_result, iterations), '
                   'offsetof(vk_skeleton_result, converged), VK_ABI_VERSION, VK_SKEL_LINKS, VK_SKEL_FILL_IN); return 0; }\n')
    exe = tmp_path / "sizeof_skel"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["32", "8", "12", "16", "20", "24", "28", "160", "48", "152", "156", "5", "13", "4"], out


def test_the_binding_matches_and_every_export_resolves(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert (C.sizeof(N.VkSkeletonRequest), C.sizeof(N.VkSkeletonResult)) == (32, 160)
    assert [f[0] for f in N.VkSkeletonRequest._fields_] == ["lo", "hi", "mode", "flags", "max_iterations", "fill_in", "fill_out", "pad"]
    assert [f[0] for f in N.VkSkeletonResult._fields_] == ["n_foreground", "n_skeleton", "n_isolated", "n_end", "n_regular", "n_junction", "links", "iterations", "converged"]
    assert (N.VkSkeletonRequest.fill_in.offset, N.VkSkeletonResult.links.offset, N.VkSkeletonResult.iterations.offset, N.VkSkeletonResult.converged.offset) == (20, 48, 152, 156)
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert "vk_skeletonize" in declared and declared == set(N.SYMBOLS), declared ^ set(N.SYMBOLS)
    assert hip_built.vk_skeletonize is not None
    # a NULL context: an error, the outputs untouched
    req, res, cls = N.VkSkeletonRequest(), SH.fresh_result(N), np.full(8, 9, np.uint8)
    assert hip_built.vk_skeletonize(None, C.byref(req), None, cls.ctypes.data, None, C.byref(res)) == -1
    assert (cls == 9).all() and (SH.result_array(res) == 7).all()


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context
    from vokselis_amd.skeleton import link_offsets, skeleton_request

    assert (V.SKEL_CURVE, V.SKEL_KERNEL, V.SKEL_CLIP_BOX, V.SKEL_INSTALL, V.SKEL_FILL_IN, V.SKEL_LINKS) == (0, 1, 1, 2, 4, 13)
    assert (V.SKEL_OFF, V.SKEL_ISOLATED, V.SKEL_END, V.SKEL_REGULAR, V.SKEL_JUNCTION) == (0, 1, 2, 3, 4)
    for name in ("SKEL_CURVE", "SKEL_KERNEL", "SKEL_CLIP_BOX", "SKEL_INSTALL", "SKEL_FILL_IN", "SKEL_JUNCTION", "SKEL_LINKS", "VkSkeletonRequest", "VkSkeletonResult", "Skeleton",
                 "skeleton_request"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.skeletonize)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("mode", "curve"), ("max_iterations", 0), ("fill_in", None),
                                                                                 ("fill_out", 0.0), ("box", None), ("install", True), ("classes", False), ("out", False)]
    r = skeleton_request(0.3, mode="kernel", max_iterations=7, fill_in=0.5, fill_out=0.25, box="clip")
    assert (r.lo, r.hi, r.mode, r.flags, r.max_iterations, r.fill_in, r.fill_out, r.pad) == (np.float32(0.3), math.inf, 1, 7, 7, 0.5, 0.25, 0)
    r = skeleton_request(0.2, 0.4, install=False)
    assert (r.mode, r.flags, r.max_iterations, r.fill_in, r.fill_out) == (0, 0, 0, 0.0, 0.0)
    assert skeleton_request(0.2, fill_in=0.0).flags == V.SKEL_INSTALL | V.SKEL_FILL_IN
    for bad in (dict(mode="surface"), dict(mode=0), dict(max_iterations=-1), dict(max_iterations=1.5), dict(max_iterations=2 ** 32)):
        with pytest.raises(ValueError):
            skeleton_request(0.3, **bad)
    # the derived values: the offsets above the centre in their order, and the length over them
    assert link_offsets()[0] == (1, 0, 0) and link_offsets()[2] == (0, 1, 0) and link_offsets()[-1] == (1, 1, 1) and len(link_offsets()) == 13 and link_offsets()[8] == (0, 0, 1)
    links = [0] * 13
    links[0], links[2], links[8], links[12] = 3, 2, 1, 4
    res = V.VkSkeletonResult(100, 11, 0, 2, 8, 1, (C.c_uint64 * 13)(*links), 6, 1)
    k = V.Skeleton(res)
    assert (k.n_foreground, k.n_skeleton, k.n_isolated, k.n_end, k.n_regular, k.n_junction, k.iterations, k.converged, k.classes, k.dense) == (100, 11, 0, 2, 8, 1, 6, True, None, None)
    assert k.links == tuple(links) and k.length() == pytest.approx(3 + 2 + 1 + 4 * math.sqrt(3.0), rel=1e-15)
    assert k.length((2.0, 3.0, 5.0)) == pytest.approx(3 * 2 + 2 * 3 + 1 * 5 + 4 * math.sqrt(4.0 + 9.0 + 25.0), rel=1e-15)


@pytest.fixture(scope="module")
def fuzz_exes(tmp_path_factory):
    """skel_fuzz twice: under ASan + UBSan, and unsanitized at -O2 for the run over all 2^26 masks."""
    out = tmp_path_factory.mktemp("skel_fuzz")
    exes = {}
    for name, c_flags in (("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), ("plain", ["-O2"])):
        obj, exe = str(out / f"skel_restatement_{name}.o"), str(out / f"skel_fuzz_{name}")
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-ffp-contract=off"] + c_flags + ["-c", "-o", obj, os.path.join(ROOT, "tests", "skel_restatement.c")], check=True)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + c_flags + ["-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "skel_fuzz.cpp"), obj, "-lm"], check=True)
        exes[name] = exe
    return exes


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261021"])
def test_validation_order_masks_tiles_and_the_replayed_iterations_under_sanitizers(fuzz_exes, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exes["san"], "60", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (60 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_the_simple_point_test_is_the_plain_flood_fill_on_all_2_to_the_26_masks(fuzz_exes):
    """The unsanitized second build over every mask (what was done: all 2^26, not the subset; just under a minute on one CPU core):
    25 985 144 masks, 38.7 %, are simple."""
    r = subprocess.run([fuzz_exes["plain"], "20", "4242", "all"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "simple: 67108864 masks tested (all 2^26), 25985144 simple" in r.stdout and r.stdout.strip().endswith("OK (20 cases)")


@pytest.fixture(scope="module")
def bonsai():
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(ROOT, "vokselis_amd", "_lib", "bonsai")
    assert os.path.exists(exe)
    return exe


NEEDS_RANGE = "--skeleton needs a value range: --components LO HI, or --iso V for [V, inf)"


@pytest.mark.parametrize("args, message", [
    (["--skeleton"], NEEDS_RANGE), (["--skeleton", "kernel", "3"], NEEDS_RANGE), (["--skeleton", "curve", "--morph-spacing", "1", "1", "2"], NEEDS_RANGE),
    (["--iso", "0.3", "--skeleton", "surface"], "--skeleton [curve|kernel] [MAX_ITER]: the mode is curve or kernel"),
    (["--iso", "0.3", "--skeleton", "kernel", "-1"], "--skeleton [curve|kernel] [MAX_ITER]: MAX_ITER is an integer >= 0"),
    (["--iso", "0.3", "--skeleton", "curve", "2.5"], "--skeleton [curve|kernel] [MAX_ITER]: MAX_ITER is an integer >= 0"),
    (["--iso", "0.3", "--skeleton", "--skeleton", "kernel"], "--skeleton: at most once"),
    (["--skeleton", "--iso", "0.3", "--gpus", "2"], "--skeleton runs on one GPU"),
    (["--morph-spacing", "1", "1", "1", "--iso", "0.3"], "--morph-spacing needs --morph"),
    (["--label-fill", "0.5", "--iso", "0.3"], "--label-fill needs a flag that drops voxels"),
])
def test_bonsai_refuses_bad_skeleton_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
