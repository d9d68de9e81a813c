"""The two references of vk_geodesic_distance held together over the shared cases (tests/geo_cases.py): the C
restatement (tests/geo_restatement.c: Dijkstra's algorithm with a binary heap) and the numpy reference (tests/np_geo_reference.py: sweeps
of the whole array with shifted minima) -- g, dense array and totals, bit for bit; the fixed cases with their pinned numbers.  The
conditions on the case list are asserted on the restatement's output, so the list cannot quietly degenerate.  The host side -- the C
boundary, vk_geo.hpp under ASan + UBSan (tests/geo_fuzz.cpp, a stand-alone program), the Python surface, the path back to a source,
bonsai's argument handling -- needs no GPU either."""
import collections
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dist_cases as DC
import geo_cases as GC
import geo_helpers as GH
import np_geo_reference as NG
import np_label_reference as NL

ROOT = GH.ROOT
G_INF, G_FAR = 0xFFFFFFFF, 0xFFFFFFFE
X0, X1 = 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return GH.build_restatement(tmp_path_factory.mktemp("geo_fuzz_cpu"))


@pytest.fixture(scope="module")
def restated(lib):
    return {c.name: GH.restate_case(lib, c) for c in GC.cases()}


def _dims(c):
    return tuple(reversed(c.vol.shape))


def _bfs_steps(s, start, conn):
    """The fewest steps from `start` (x, y, z) to every voxel of s, by a plain breadth-first search; -1 where there is no path."""
    nz, ny, nx = s.shape
    steps = np.full(s.shape, -1, np.int64)
    steps[start[2], start[1], start[0]] = 0
    queue = collections.deque([start])
    offs = NL.offsets(conn)
    while queue:
        x, y, z = queue.popleft()
        for dz, dy, dx in offs:
            ux, uy, uz = x + dx, y + dy, z + dz
            if 0 <= ux < nx and 0 <= uy < ny and 0 <= uz < nz and s[uz, uy, ux] and steps[uz, uy, ux] < 0:
                steps[uz, uy, ux] = steps[z, y, x] + 1
                queue.append((ux, uy, uz))
    return steps


def test_case_list_covers_the_issue(restated, lib):
    import vokselis_amd as V

    cases = GC.cases()
    assert len({c.name for c in cases}) == len(cases) and 100 <= len(cases) <= 200, len(cases)
    assert max(c.vol.size for c in cases) <= GC.MAX_VOXELS
    src = open(os.path.join(ROOT, "vokselis_amd", "csrc", "vk_label.hpp")).read()
    assert tuple(int(v) for v in re.search(r"kLabelTile = \{(\d+)u, (\d+)u, (\d+)u,", src).groups()) == GC.TILE == (32, 16, 8)
    dims = {_dims(c) for c in cases}
    assert set(GC.DIMS) | {GC.BIG, (37, 21, 11), (12, 7, 3), (5, 1, 1)} <= dims
    assert all(any(d[a] == 1 for d in dims) for a in range(3))                                                  # 1 on each axis in turn
    assert any(all(n % t for n, t in zip(d, GC.TILE)) for d in dims) and any(all(n % t == 0 for n, t in zip(d, GC.TILE)) for d in dims)
    assert all(n > 2 * t for n, t in zip(GC.BIG, GC.TILE))                                                      # 3 x 3 x 3 tiles
    for kind in ("u8", "u16", "f16"):
        mine = [c for c in cases if c.kind == kind]
        text = " | ".join(c.name for c in mine)
        for word in ("empty,", "full,", "no source on the set", "seeds alone", "a seed plus a face", "a seed on the set and a seed off it", "unreachable pocket", "serpentine",
                     "the cheap detour", "the late shortcut", "density 0.31", "density 0.6", "density 0.9", ", box (", "clip box", "empty box", "uniform noise", "the fixed set"):
            assert word in text, (kind, word)
        assert {c.conn for c in mine} == {6, 18, 26} and {c.spacing for c in mine} >= set(GC.SPACINGS)
        assert {c.gain == 0.0 for c in mine} == {True, False}                                                   # automatic and fixed gain
        assert set(GC.FACE.values()) <= {c.sources for c in mine}                                               # every face as the source at least once
        assert any(c.sources == 0 and c.seeds for c in mine) and any(c.sources and c.seeds for c in mine)
    special = [c for c in cases if "NaN, inf" in c.name]
    assert {(c.lo, c.hi) for c in special} >= {(-math.inf, math.inf), (math.inf, math.inf), (-math.inf, -math.inf), (0.0, 0.0)}
    # what the cases exercise, on the restatement's output: result = n_foreground, n_sources, n_reached, n_saturated, n_target_reached, sum_g, max_g, target_min, gain
    by = {c.name: (c, restated[c.name]) for c in cases}

    def one(word, kind="u8", **where):
        return next((c, r) for c, r in by.values() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))

    c, r = one("empty,")
    assert not r[2][:7].any() and int(r[2][7]) == G_INF and int(r[2][8]) == 0 and (r[0] == G_INF).all()         # the empty set: nothing, and the automatic gain is 0
    c, r = one("full,", conn=26)
    assert int(r[2][0]) == c.vol.size == int(r[2][2]) and int(r[2][1]) == 37 * 21 and int(r[2][7]) == 10 * 256   # a full set from z+: the straight way to z-
    c, r = one("no source on the set")
    assert int(r[2][0]) > 0 and not r[2][1:7].any() and int(r[2][7]) == G_INF and (r[0] == G_INF).all()
    c, r = one("a seed on the set and a seed off it")
    assert int(r[2][1]) == 1 and int(r[2][2]) == int(r[2][0]) > 0 and r[0][0, 0, 0] == G_INF                      # the seed off S contributes nothing
    c, r = one("unreachable pocket", conn=26)
    assert 0 < int(r[2][2]) < int(r[2][0]) and int(r[2][7]) == G_INF and int(r[2][4]) == 0                       # the far block is never reached: no percolation
    assert all(int(r[2][3]) == 0 for _, r in by.values())                                                       # no case saturates (the host fuzz covers VK_GEO_FAR)
    assert sum(0 < int(r[2][2]) < int(r[2][0]) for _, r in by.values()) > 15                                    # reached and unreached voxels in one case
    # the serpentine: the path from its far end enters the tile at the origin at least four times
    c, r = one("serpentine", conn=6)
    far = np.unravel_index(np.argmax(np.where(r[0] == G_INF, 0, r[0])), r[0].shape)
    path = V.geodesic_path(r[0], (far[2], far[1], far[0]), c.spacing, c.conn)
    tiles = [GH.tile_of(p) for p in path]
    entries = sum(1 for a, b in zip(tiles, tiles[1:]) if a != b and b == (0, 0, 0)) + (tiles[0] == (0, 0, 0))
    assert entries >= 4 and len(path) > 300 and int(r[2][2]) == int(r[2][0]), entries
    # the cheap detour: the shortest path has more steps than the fewest-steps path
    d, m, seed, goal = GC.detour()
    for conn in (6, 26):
        c, r = one("the cheap detour", conn=conn)
        assert c.spacing[2] >= 8 and c.spacing[:2] == (1, 1)
        path = V.geodesic_path(r[0], goal, c.spacing, c.conn)
        fewest = int(_bfs_steps(m, seed, conn)[goal[2], goal[1], goal[0]])
        assert 0 < fewest < len(path) - 1, (conn, fewest, len(path))
    # the late shortcut: the route with fewer tile crossings is the longer one
    d, m, seed, goal = GC.shortcut()
    c, r = one("the late shortcut", conn=6)
    short = V.geodesic_path(r[0], goal, c.spacing, 6)
    blocked = GH.restate(lib, DC.mask_volume(GC.shortcut(blocked=True)[1], "u8"), "u8", c.lo, c.hi, 6, c.spacing, 0, X1, (seed,))
    long = V.geodesic_path(blocked[0], goal, c.spacing, 6)
    assert GH.tile_crossings(short) == 3 and GH.tile_crossings(long) == 1 and len(long) > 3 * len(short) and int(blocked[0][goal[2], goal[1], goal[0]]) > 3 * int(r[0][goal[2], goal[1], goal[0]])


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(restated):
    for c in GC.cases():
        assert GH.differences(restated[c.name], GH.reference_case(c)) == "", c.name


def test_the_fixed_cases_give_the_pinned_numbers(lib):
    vol = DC.mask_volume(GC.fixed_mask(), "u8")
    assert int(GC.fixed_mask().sum()) == 206
    pinned = {(6, (1, 1, 1)): (5888, 531968, 4352), (6, (1, 1, 3)): (5888, 531968, 4352), (6, (2, 1, 1)): (8704, 826624, 7168),
              (18, (1, 1, 1)): (4838, 461018, 3902), (18, (1, 1, 3)): (4838, 461018, 3902), (18, (2, 1, 1)): (7332, 733916, 6580),
              (26, (1, 1, 1)): (4838, 460949, 3902), (26, (1, 1, 3)): (4838, 461018, 3902), (26, (2, 1, 1)): (7332, 733775, 6580)}
    for (conn, spacing), (max_g, sum_g, target_min) in pinned.items():
        for got in (GH.restate(lib, vol, "u8", 0.5, math.inf, conn, spacing, X0, X1), NG.apply(vol, "u8", 0.5, math.inf, conn, spacing, X0, X1, (), 0.0, 0.0, 0.0, None)):
            r = [int(v) for v in got[2]]
            assert r[0] == 206 and r[2] == 206 and (r[6], r[5], r[7]) == (max_g, sum_g, target_min), (conn, spacing, r)
    vol = DC.mask_volume(GC.second_fixed_mask(), "u8")
    for got in (GH.restate(lib, vol, "u8", 0.5, math.inf, 6, (1, 1, 1), X0, X1), NG.apply(vol, "u8", 0.5, math.inf, 6, (1, 1, 1), X0, X1, (), 0.0, 0.0, 0.0, None)):
        assert got[0].ravel().tolist() == [0, 256, G_INF, G_INF, G_INF] and int(got[2][2]) == 2 and int(got[2][0]) - int(got[2][2]) == 2 and int(got[2][7]) == G_INF


# ---- the path back to a source, and the derived values --------------------------------------------------------------------------------
def test_geodesic_path_ends_on_a_source_and_its_costs_sum_to_g(lib):
    import vokselis_amd as V

    vol = DC.mask_volume(GC.fixed_mask(), "u8")
    for conn, spacing in ((6, (1, 1, 1)), (18, (1, 1, 3)), (26, (2, 1, 1)), (26, (1, 2, 3))):
        for got in (GH.restate(lib, vol, "u8", 0.5, math.inf, conn, spacing, X0, X1), NG.apply(vol, "u8", 0.5, math.inf, conn, spacing, X0, X1, (), 0.0, 0.0, 0.0, None)):
            g = got[0]
            for z, y, x in np.argwhere(g != G_INF)[::7]:
                path = V.geodesic_path(g, (x, y, z), spacing, conn)
                assert tuple(path[0]) == (x, y, z) and g[path[-1][2], path[-1][1], path[-1][0]] == 0 and path[-1][0] == 0      # ends on the face x-
                cost = sum(NG.step_cost(spacing, *(int(v) for v in (b - a))) for a, b in zip(path, path[1:]))
                assert cost == int(g[z, y, x]) and all(GC.fixed_mask()[p[2], p[1], p[0]] for p in path)
                assert all(1 <= int(np.abs(b - a).sum()) <= {6: 1, 18: 2, 26: 3}[conn] and int(np.abs(b - a).max()) == 1 for a, b in zip(path, path[1:]))
    # 17 unit steps at connectivity 6 from the nearest target voxel of the fixed case
    g = GH.restate(lib, vol, "u8", 0.5, math.inf, 6, (1, 1, 1), X0, X1)[0]
    on_face = np.argwhere(g[:, :, 11] == g[:, :, 11].min())[0]
    path = V.geodesic_path(g, (11, on_face[1], on_face[0]), (1, 1, 1), 6)
    assert int(g[:, :, 11].min()) == 4352 == 17 * 256 and len(path) == 18
    # a tie takes the smallest offset index: from (1, 1, 0) of a full plane under connectivity 26 at pitch (1, 1, 1) there is one way, straight; at (2, 0, 0) ...
    full = np.zeros((1, 3, 3), np.uint32)
    full[0] = [[0, 256, 512], [0, 256, 512], [0, 256, 512]]
    assert V.geodesic_path(full, (2, 1, 0), (1, 1, 1), 6).tolist() == [[2, 1, 0], [1, 1, 0], [0, 1, 0]]
    tie = np.array([[[0, 256, 0]]], np.uint32)
    assert V.geodesic_path(tie, (1, 0, 0), (1, 1, 1), 6).tolist() == [[1, 0, 0], [0, 0, 0]]                        # offset 12 (dx = -1) before offset 14
    for bad in (G_INF, G_FAR):
        with pytest.raises(ValueError):
            V.geodesic_path(np.array([[[0, bad]]], np.uint32), (1, 0, 0))
    with pytest.raises(ValueError):
        V.geodesic_path(tie, (3, 0, 0))


def test_geodesic_derived_values_on_the_fixed_case(lib):
    import vokselis_amd as V

    vol = DC.mask_volume(GC.fixed_mask(), "u8")
    g, dense, r = GH.restate(lib, vol, "u8", 0.5, math.inf, 6, (1, 1, 1), X0, X1)
    res = V.VkGeodesicResult(*[int(v) for v in r[:8]], float(np.uint32(r[8]).view(np.float32)), 0)
    t = V.Geodesic(res, (1, 1, 1), (12, 7, 3), g, dense)
    assert (t.n_foreground, t.n_sources, t.n_reached, t.n_unreached, t.n_saturated, t.max_g, t.sum_g, t.target_min) == (206, 21, 206, 0, 0, 5888, 531968, 4352)
    assert t.reached_fraction == 1.0 and t.percolates and t.max_distance == 23.0 and t.target_distance == 17.0 and t.mean_distance == 531968 / (256 * 206)
    assert t.tortuosity("x") == 17 / 11 == t.tortuosity(0) and t.gain == float(np.float32(1.0) / np.float32(5888))
    assert t.distance.dtype == np.float64 and t.distance.max() == math.inf and t.distance[g != G_INF].max() == 23.0 and t.g is g and t.dense is dense
    with pytest.raises(ValueError):
        V.Geodesic(res, (1, 1, 1), (12, 7, 1)).tortuosity("z")
    g, dense, r = GH.restate(lib, DC.mask_volume(GC.second_fixed_mask(), "u8"), "u8", 0.5, math.inf, 6, (1, 1, 1), X0, X1)
    t = V.Geodesic(V.VkGeodesicResult(*[int(v) for v in r[:8]], 0.0, 0), (1, 1, 1), (5, 1, 1))
    assert (t.n_reached, t.n_unreached, t.percolates, t.target_distance, t.tortuosity("x"), t.reached_fraction, t.distance) == (2, 2, False, math.inf, math.inf, 0.5, None)
    empty = V.Geodesic(V.VkGeodesicResult(0, 0, 0, 0, 0, 0, 0, G_INF, 0.0, 0))
    assert (empty.reached_fraction, empty.mean_distance, empty.max_distance, empty.percolates) == (0.0, 0.0, 0.0, False)


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    for name, value in (("VK_GEO_INF", "0xFFFFFFFFu"), ("VK_GEO_FAR", "0xFFFFFFFEu"), ("VK_GEO_UNIT", "256u"), ("VK_GEO_MAX_SEEDS", "16")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert "enum { VK_GEO_CLIP_BOX = 1, VK_GEO_INSTALL = 2 };" in code
    assert "enum { VK_GEO_FACE_X0 = 1, VK_GEO_FACE_X1 = 2, VK_GEO_FACE_Y0 = 4, VK_GEO_FACE_Y1 = 8, VK_GEO_FACE_Z0 = 16, VK_GEO_FACE_Z1 = 32 };" in code
    assert re.search(r"int vk_geodesic_distance\(vk_ctx \*ctx, const vk_geodesic_request \*req, const vk_voxel_box \*box, uint32_t \*g_out, void \*dense_out,\s*"
                     r"vk_geodesic_result \*result\);", code)
    assert "static_assert(sizeof(vk_geodesic_request) == 248 && sizeof(vk_geodesic_result) == 64" in code
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 30\. ", design, flags=re.M)
    section = design[design.index("## 30. "):]
    for phrase in ("min(a + w, VK_GEO_FAR)", "VK_GEO_INSTALL", "16384, 23170 and 28377"):
        assert phrase in _header(), phrase
        assert phrase in section, phrase
    for word in ("Stale reads", "The active set", "Resources", "Measurements", "Checks", "Hosts", "Out of scope", "no device case saturates"):
        assert word in section, word
    assert "vk_geodesic_distance" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "geodesic_distance" in open(os.path.join(ROOT, "README.md")).read() and "--geodesic" in open(os.path.join(ROOT, "README.md")).read()
    assert "geo_quick.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "geo_pass_isa.txt"))


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_geo.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(vk_geodesic_request), offsetof(vk_geodesic_request, connectivity), '
                   'offsetof(vk_geodesic_request, spacing), offsetof(vk_geodesic_request, source_faces), offsetof(vk_geodesic_request, n_seeds), offsetof(vk_geodesic_request, gain), '
                   'offsetof(vk_geodesic_request, fill_unreached), offsetof(vk_geodesic_request, pad), offsetof(vk_geodesic_request, seeds), sizeof(vk_geodesic_result), '
                   'offsetof(vk_geodesic_result, sum_g), offsetof(vk_geodesic_result, max_g), offsetof(vk_geodesic_result, gain), VK_ABI_VERSION, VK_GEO_MAX_SEEDS, VK_GEO_INSTALL); return 0; }\n')
    exe = tmp_path / "sizeof_geo"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["248", "8", "16", "28", "36", "40", "48", "52", "56", "64", "40", "48", "56", "5", "16", "2"], out


def test_the_binding_matches_and_every_export_resolves(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert (C.sizeof(N.VkGeodesicRequest), C.sizeof(N.VkGeodesicResult)) == (248, 64)
    assert [f[0] for f in N.VkGeodesicRequest._fields_] == ["lo", "hi", "connectivity", "flags", "spacing", "source_faces", "target_faces", "n_seeds", "gain", "fill_out", "fill_unreached", "pad",
                                                            "seeds"]
    assert [f[0] for f in N.VkGeodesicResult._fields_] == ["n_foreground", "n_sources", "n_reached", "n_saturated", "n_target_reached", "sum_g", "max_g", "target_min", "gain", "pad"]
    assert (N.VkGeodesicRequest.spacing.offset, N.VkGeodesicRequest.gain.offset, N.VkGeodesicRequest.seeds.offset, N.VkGeodesicResult.max_g.offset, N.VkGeodesicResult.gain.offset) == (16, 40, 56, 48, 56)
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert "vk_geodesic_distance" in declared and declared == set(N.SYMBOLS), declared ^ set(N.SYMBOLS)
    assert hip_built.vk_geodesic_distance is not None
    # a NULL context: an error, the outputs untouched
    req, res, g = N.VkGeodesicRequest(), GH.fresh_result(N), np.full(8, 9, np.uint32)
    assert hip_built.vk_geodesic_distance(None, C.byref(req), None, g.ctypes.data, None, C.byref(res)) == -1
    assert (g == 9).all() and res.n_foreground == 7 and res.max_g == 7


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context
    from vokselis_amd.geodesic import geodesic_request

    assert (V.GEO_INF, V.GEO_FAR, V.GEO_UNIT, V.GEO_MAX_SEEDS, V.GEO_CLIP_BOX, V.GEO_INSTALL) == (G_INF, G_FAR, 256, 16, 1, 2)
    assert (V.GEO_FACE_X0, V.GEO_FACE_X1, V.GEO_FACE_Y0, V.GEO_FACE_Y1, V.GEO_FACE_Z0, V.GEO_FACE_Z1) == (1, 2, 4, 8, 16, 32)
    for name in ("GEO_INF", "GEO_FAR", "GEO_UNIT", "GEO_MAX_SEEDS", "GEO_CLIP_BOX", "GEO_INSTALL", "GEO_FACE_X0", "GEO_FACE_Z1", "VkGeodesicRequest", "VkGeodesicResult", "Geodesic",
                 "geodesic_request", "geodesic_path"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.geodesic_distance)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("sources", ("x-",)), ("seeds", ()), ("targets", ()),
                                                                                 ("connectivity", 26), ("spacing", (1, 1, 1)), ("gain", 0.0), ("fill_out", 0.0), ("fill_unreached", 0.0),
                                                                                 ("box", None), ("install", True), ("out", False), ("g", False)]
    r = geodesic_request(0.3, sources=("x-", "z+"), seeds=((1, 2, 3), (4, 5, 6)), targets=("y+",), connectivity=18, spacing=(1, 2, 3), gain=0.125, fill_out=0.25, fill_unreached=0.5, box="clip")
    assert (r.lo, r.hi, r.connectivity, r.flags, list(r.spacing), r.source_faces, r.target_faces, r.n_seeds, r.gain, r.fill_out, r.fill_unreached, r.pad) == \
        (np.float32(0.3), math.inf, 18, 3, [1, 2, 3], 33, 8, 2, 0.125, 0.25, 0.5, 0)
    assert [list(s) for s in r.seeds][:3] == [[1, 2, 3], [4, 5, 6], [0, 0, 0]]
    r = geodesic_request(0.2, 0.4, install=False)
    assert (r.flags, r.connectivity, list(r.spacing), r.source_faces, r.target_faces, r.n_seeds, r.gain) == (0, 26, [1, 1, 1], 1, 0, 0, 0.0)
    assert geodesic_request(0.2, sources="y-", targets="y+").source_faces == 4
    for bad in (dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(spacing=(1, 65, 1)), dict(spacing=(1.5, 1, 1)), dict(connectivity=8), dict(sources=("w-",)), dict(targets=("x",)),
                dict(seeds=((1, 2),)), dict(seeds=((1, 2, -3),)), dict(seeds=((0, 0, 0),) * 17), dict(gain=-1.0), dict(gain=math.inf), dict(gain=math.nan)):
        with pytest.raises(ValueError):
            geodesic_request(0.3, **bad)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geo_fuzz") / "geo_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "geo_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261021"])
def test_validation_order_costs_tiles_and_the_replayed_rounds_under_sanitizers(fuzz_exe, seed):
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


NEEDS_RANGE = "--geodesic and --geodesic-voxel need a value range: --components LO HI, or --iso V for [V, inf)"
A_FACE = "--geodesic FACE [TARGET_FACE]: a face is one of x- x+ y- y+ z- z+"


@pytest.mark.parametrize("args, message", [
    (["--geodesic", "x-"], NEEDS_RANGE), (["--geodesic", "x-", "x+", "--morph-spacing", "1", "1", "2"], NEEDS_RANGE), (["--geodesic-voxel", "1", "2", "3"], NEEDS_RANGE),
    (["--geodesic", "left", "--iso", "0.3"], A_FACE), (["--geodesic", "x-", "up", "--iso", "0.3"], A_FACE), (["--geodesic", "X-", "--iso", "0.3"], A_FACE),
    (["--geodesic"], "missing value for --geodesic"), (["--iso", "0.3", "--geodesic-voxel", "1", "2"], "missing value for --geodesic-voxel"),
    (["--iso", "0.3", "--geodesic", "x-", "--geodesic", "y-"], "--geodesic: at most once"),
    (["--iso", "0.3", "--geodesic-voxel", "1", "-2", "3"], "--geodesic-voxel X Y Z: three voxel indices >= 0"),
    (["--iso", "0.3"] + ["--geodesic-voxel", "1", "2", "3"] * 17, "--geodesic-voxel: at most 16 seeds"),
    (["--geodesic", "x-", "x+", "--iso", "0.3", "--gpus", "2"], "--geodesic runs on one GPU"), (["--geodesic-voxel", "1", "2", "3", "--components", "0.3", "inf", "18", "--gpus", "2"], "run on one GPU"),
    (["--morph-spacing", "1", "1", "1", "--iso", "0.3"], "--morph-spacing needs --morph"),
    (["--label-fill", "0.5", "--iso", "0.3"], "--label-fill needs a flag that drops voxels"),
])
def test_bonsai_refuses_bad_geodesic_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
