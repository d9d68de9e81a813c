"""The two references of vk_measure_components held together over the shared cases (tests/measure_cases.py): the C
restatement (tests/measure_restatement.c: a walk voxel by voxel, sums in __int128) and the numpy reference (tests/np_measure_reference.py:
bincounts of exact pieces) -- every word of every record, bit for bit.  The conditions on the case list are asserted, so the list cannot
quietly degenerate.  The host side -- the C boundary, vk_measure.hpp under ASan + UBSan (tests/measure_fuzz.cpp, a stand-alone program),
the Python surface and its derived quantities against a float64 computation over each region's voxels -- needs no GPU either."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import label_helpers as LH
import measure_cases as MC
import measure_helpers as MH
import np_measure_reference as NM

ROOT = LH.ROOT
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("measure_fuzz_cpu")
    return MH.build_restatement(d), LH.build_restatement(d)


@pytest.fixture(scope="module")
def restated(libs):
    return {c.name: MH.restate_case(libs[0], libs[1], c) for c in MC.cases()}


def test_case_list_covers_the_issue(libs, restated):
    cases = MC.cases()
    assert len({c.name for c in cases}) == len(cases) and 36 <= len(cases) <= 80, len(cases)
    assert max(c.vol.size for c in cases) == MC.MAX_VOXELS and {c.kind for c in cases} == {"u8", "u16", "f16"}
    dims = {tuple(reversed(c.vol.shape)) for c in cases}
    assert any(d[0] < 64 and 64 % d[0] for d in dims) and any(d[0] > 64 and d[0] % 64 for d in dims) and any(d[0] == 64 for d in dims)
    assert any((d[0] * d[1] * d[2]) % 4096 and d[0] * d[1] * d[2] > 3 * 4096 for d in dims)     # ends inside a chunk, after several
    assert {c.conn for c in cases if c.labels is None} == {6, 18, 26}
    assert any(c.box is not None and c.clip is None for c in cases) and any(c.clip is not None for c in cases)
    t = lambda c: restated[c.name][0]
    for c in cases:
        table = t(c)
        if "one region fills the volume" in c.name or "one label everywhere" in c.name:
            assert len(table) == 1 and int(table[0, 0]) == c.vol.size > 4 * 4096
        if "isolated voxels" in c.name:
            assert len(table) == 6912 > 50 * MC.SLOTS and (table[:, 0] == 1).all() and (table[:, 24:27] == 2).all()
        if "one region through the corners" in c.name:
            assert len(table) == 1 and int(table[0, 0]) == 6912
        if "an empty box" in c.name:
            assert len(table) == 0 and restated[c.name][1] == 0
        if "a region on every border" in c.name:
            b = c.box or LH.whole(c.vol)
            assert len(table) == 1 and tuple(int(v) for v in table[0, 2:8]) == tuple(b)
            ex = [b[3] - b[0], b[4] - b[1], b[5] - b[2]]
            assert [int(v) for v in table[0, 24:27]] == [2 * ex[1] * ex[2], 2 * ex[0] * ex[2], 2 * ex[0] * ex[1]]   # a block's faces
        if "every voxel 65535" in c.name:
            big = int(np.argmax(table[:, 0]))
            n = int(table[big, 0])
            assert int(table[big, 18]) == int(table[big, 19]) == 65535 and int(table[big, 23]) == n * 65535 * 65535 and int(table[big, 22]) == 0
        if "unused ids" in c.name:
            used = np.unique(c.labels[c.labels != 0])
            empty = np.setdiff1d(np.arange(1, c.max_label + 1), used) - 1
            assert len(empty) >= 5 and (table[empty, 0] == 0).all() and (table[empty, 1] == 0xFFFFFFFFFFFFFFFF).all() and (table[empty, 2:18] == 0).all()
            assert (table[empty, 18] == 0x7FFFFFFFFFFFFFFF).all() and (table[empty, 19] == 0x8000000000000000).all() and (table[empty, 20:] == 0).all()
        if "regions that share faces" in c.name:
            # a face between two regions counts once for each: every pair of neighbours (the volume padded with label 0) that differ gives one face per labelled end
            P, total, shared = np.pad(c.labels.astype(np.int64), 1), 0, 0
            for a in range(3):
                one, other = P.take(range(P.shape[a] - 1), a), P.take(range(1, P.shape[a]), a)
                differ = one != other
                total += int((differ & (one > 0)).sum()) + int((differ & (other > 0)).sum())
                shared += int((differ & (one > 0) & (other > 0)).sum())
            assert shared > 100 and int(table[:, 24:27].sum()) == total
        if "a region with no finite voxel" in c.name:
            assert int(table[1, 0]) == int(table[1, 17]) > 50 and int(table[1, 18]) == 0x7FFFFFFFFFFFFFFF and int(table[1, 19]) == 0x8000000000000000 and (table[1, 20:24] == 0).all()
            assert int(table[0, 18]) == 0 and int(table[0, 19]) == 1 and int(table[2, 0]) == 0   # -0 and the smallest subnormal: q = 0 and 1; id 3 is unused
    ext = [c for c in cases if "extremes" in c.name and c.lo == -math.inf and c.hi == math.inf][0]
    bits = ext.vol.view(np.uint16)
    assert all((bits == b).any() for b in (0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x8000, 0x7C00, 0xFC00, 0x7E00))
    table = t(ext)
    assert int(table[:, 17].sum()) == int(((bits & 0x7FFF) == 0x7C00).sum()) > 100          # the infinities are in the range; no NaN is
    assert int(table[:, 18].min().astype(np.int64)) == -(65504 << 24) and int(table[:, 19].astype(np.int64).max()) == 65504 << 24
    wide = t([c for c in cases if "the widest sums" in c.name][0])
    n = int(wide[0, 0])
    assert (int(wide[0, 22]) << 64) + int(wide[0, 23]) == n * (65504 << 24) ** 2 > 1 << 64 and int(wide[0, 22]) > 0   # sum_qq needs its high word


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(libs, restated):
    for c in MC.cases():
        ref, fg = MH.reference_case(libs[1], c)
        assert MH.differences(restated[c.name][0], ref) == "" and restated[c.name][1] == fg, c.name


def test_an_id_above_the_regions_is_refused_by_the_restatement_too(libs):
    c = next(c for c in MC.cases() if "unused ids" in c.name)
    v, lab, table, fg = np.ascontiguousarray(c.vol), c.labels, np.zeros((4, MH.COLS), np.uint64), C.c_uint64(0)
    rc = libs[0].measure_restate(C.c_void_p(v.ctypes.data), C.c_uint32(v.shape[2]), C.c_uint32(v.shape[1]), C.c_uint32(v.shape[0]), C.c_int(LH.FMT[c.kind]), C.c_void_p(lab.ctypes.data),
                                 C.c_uint64(4), C.c_void_p(table.ctypes.data), C.byref(fg))
    assert rc == 2


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert "enum { VK_MEASURE_CLIP_BOX = 1 };" in code
    assert re.search(r"int vk_measure_components\(vk_ctx \*ctx, const vk_measure_request \*req, const vk_voxel_box \*box, const uint32_t \*labels_in, vk_region \*regions,\s*"
                     r"uint64_t cap_regions, vk_measure_result \*result\);", code)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 28\. ", design, flags=re.M)
    section = design[design.index("## 28. "):]
    for word in ("Visibility", "Termination", "Out of scope", "labels_in", "n_nonfinite", "faces"):
        assert word in section, word
    assert "vk_measure_components" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "measure_pass_isa.txt"))


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_measure.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(vk_measure_request), offsetof(vk_measure_request, connectivity), '
                   'offsetof(vk_measure_request, max_label), sizeof(vk_region), offsetof(vk_region, box), offsetof(vk_region, sum_x), offsetof(vk_region, sum_xx), '
                   'offsetof(vk_region, n_nonfinite), offsetof(vk_region, q_min), offsetof(vk_region, sum_q_hi), offsetof(vk_region, sum_qq_hi), offsetof(vk_region, faces), '
                   'sizeof(vk_measure_result), offsetof(vk_measure_result, scale), VK_ABI_VERSION, VK_MEASURE_CLIP_BOX); return 0; }\n')
    exe = tmp_path / "sizeof_measure"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["24", "8", "16", "192", "16", "40", "64", "112", "120", "136", "152", "168", "32", "24", "5", "1"], out


def test_the_binding_matches_and_every_export_resolves(hip_built):
    from vokselis_amd import _native as N
    from vokselis_amd.measure import REGION_DTYPE

    assert hip_built.vk_abi_version() == 5
    assert (C.sizeof(N.VkMeasureRequest), C.sizeof(N.VkRegion), C.sizeof(N.VkMeasureResult)) == (24, 192, 32)
    assert [f[0] for f in N.VkMeasureRequest._fields_] == ["lo", "hi", "connectivity", "flags", "max_label", "pad"]
    assert [f[0] for f in N.VkMeasureResult._fields_] == ["n_regions", "n_foreground", "records_written", "scale", "pad"]
    for name, offset in (("box", 16), ("sum_x", 40), ("sum_xx", 64), ("n_nonfinite", 112), ("q_min", 120), ("sum_q_hi", 136), ("sum_qq_hi", 152), ("faces", 168)):
        assert getattr(N.VkRegion, name).offset == offset, name
    assert REGION_DTYPE.itemsize == 192 and [REGION_DTYPE.fields[k][1] for k in ("box", "sums", "n_nonfinite", "q_min", "sum_q_hi", "sum_qq_hi", "faces")] == [16, 40, 112, 120, 136, 152, 168]
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert "vk_measure_components" in declared and declared == set(N.SYMBOLS), declared ^ set(N.SYMBOLS)
    assert hip_built.vk_measure_components is not None
    # a NULL context: an error, the outputs untouched
    req, res, regions = N.VkMeasureRequest(), N.VkMeasureResult(), (N.VkRegion * 2)()
    res.n_regions = 7
    C.memset(regions, 0xAB, C.sizeof(regions))
    assert hip_built.vk_measure_components(None, C.byref(req), None, None, regions, 2, C.byref(res)) == -1
    assert bytes(regions) == b"\xab" * C.sizeof(regions) and res.n_regions == 7


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context

    assert V.MEASURE_CLIP_BOX == 1
    for name in ("MEASURE_CLIP_BOX", "VkMeasureRequest", "VkRegion", "VkMeasureResult", "Measurements", "measure_request"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.measure_components)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", None), ("hi", math.inf), ("connectivity", 6), ("box", None), ("labels", None), ("max_label", None)]
    r = V.measure_request(0.3, connectivity=26, box="clip")
    assert (r.lo, r.hi, r.connectivity, r.flags, r.max_label, r.pad) == (np.float32(0.3), math.inf, 26, 1, 0, 0)
    r = V.measure_request(max_label=9)
    assert (r.lo, r.hi, r.connectivity, r.flags, r.max_label, r.pad) == (0.0, 0.0, 0, 0, 9, 0)
    for bad in (dict(max_label=0), dict(max_label=1.5), dict(max_label=1 << 32), dict(max_label=3, box="clip")):
        with pytest.raises(ValueError):
            V.measure_request(**bad)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("measure_fuzz") / "measure_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "measure_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261020"])
def test_validation_overflow_bound_limbs_runs_and_records_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "300", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (300 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- the derived quantities -----------------------------------------------------------------------------------------------------------
def _measurements(c, table, fg):
    """A Measurements from a restatement's table, as Context.measure_components builds one from the library's."""
    from vokselis_amd import _native as N
    from vokselis_amd.measure import Measurements

    res = N.VkMeasureResult()
    res.n_regions, res.n_foreground, res.records_written, res.scale = len(table), fg, len(table), NM.SCALE[c.kind]
    return Measurements(MH.regions_from_table(table), len(table), res, tuple(reversed(c.vol.shape)))


def test_derived_quantities_against_float64_over_each_regions_voxels(libs, restated):
    """The values under test are one rounding away from exact integers, so the whole tolerance is the float64 reference's own error, derived
    per quantity from the standard bound of a recursive sum of n terms, n eps sum |terms|:
      centroid   ref = sum(x) / n:                        d_c = n eps sum|x| / n
      covariance ref = sum((x - cx)(y - cy)) / n:         n eps sum|(x - cx)(y - cy)| / n + d_cx mean|y - cy| + d_cy mean|x - cx|   (the centroids' own error, first order)
      mean       ref = sum(v) / m, v = q / scale rounded: d_m = (m + 2) eps sum|v| / m
      variance   ref = sum((v - mean)^2) / m:             (m + 4) eps mean((v - mean)^2) + 2 mean|v - mean| (eps max|v| + d_m)
      area       ref = the exposed faces counted in float64 times the face areas: 4 eps ref.
    A spacing of (0.5, 1.25, 2.0) -- exact in binary -- scales lengths."""
    sp = (0.5, 1.25, 2.0)
    checked = 0
    for c in MC.cases():
        table, fg = restated[c.name]
        if len(table) == 0:
            continue
        labels, n_regions, _ = MH.case_labels(libs[1], c)
        m = _measurements(c, table, fg)
        cen, cov, mean, var, std, area, vol_, lo, hi = m.centroid, m.covariance(sp), m.mean, m.variance, m.std, m.surface_area(sp), m.volume(sp), m.min, m.max
        values, vectors = m.principal_axes(sp)
        value = np.asarray(c.vol).astype(np.float64) / (1.0 if c.kind == "f16" else float(NM.SCALE[c.kind]))
        padded = np.pad(labels, 1)
        ids = list(m.largest(12)) + list(range(1, min(len(table), 6) + 1))
        for k in sorted(set(int(i) for i in ids)):
            sel = labels == k
            n = int(sel.sum())
            assert n == int(m.sizes[k - 1])
            if n == 0:
                assert np.isnan(cen[k - 1]).all() and np.isnan(cov[k - 1]).all() and math.isnan(mean[k - 1]) and math.isnan(var[k - 1]) and math.isnan(lo[k - 1]) and area[k - 1] == 0.0
                assert np.isnan(values[k - 1]).all() and not m.touches_border[k - 1]
                continue
            z, y, x = (a.astype(np.float64) for a in np.nonzero(sel))
            pos = (x, y, z)
            ref_c = [float(p.sum()) / n for p in pos]
            d_c = [n * EPS * float(np.abs(p).sum()) / n for p in pos]
            for a in range(3):
                assert abs(cen[k - 1, a] - ref_c[a]) <= d_c[a] + EPS * abs(ref_c[a]), (c.name, k, a)
            dev = [pos[a] - ref_c[a] for a in range(3)]
            for a in range(3):
                for b in range(3):
                    terms = dev[a] * dev[b]
                    ref = float(terms.sum()) / n * sp[a] * sp[b]
                    bound = (n * EPS * float(np.abs(terms).sum()) / n + d_c[a] * float(np.abs(dev[b]).mean()) + d_c[b] * float(np.abs(dev[a]).mean())) * sp[a] * sp[b]
                    assert abs(cov[k - 1, a, b] - ref) <= bound + 4 * EPS * abs(ref), (c.name, k, a, b, cov[k - 1, a, b], ref, bound)
            w = np.linalg.eigvalsh(cov[k - 1])[::-1]
            assert np.allclose(values[k - 1], w, rtol=0, atol=16 * EPS * max(abs(w).max(), 1.0)) and (np.diff(values[k - 1]) <= 0).all()
            assert np.allclose(cov[k - 1] @ vectors[k - 1], vectors[k - 1] * values[k - 1], rtol=0, atol=64 * EPS * max(abs(w).max(), 1.0))
            v = value[sel]
            v = v[np.isfinite(v)]
            assert len(v) == int(m.n_finite[k - 1])
            if len(v) == 0:
                assert math.isnan(mean[k - 1]) and math.isnan(var[k - 1]) and math.isnan(lo[k - 1]) and math.isnan(hi[k - 1])
            else:
                mm = len(v)
                ref_m = float(v.sum()) / mm
                d_m = (mm + 2) * EPS * float(np.abs(v).sum()) / mm
                assert abs(mean[k - 1] - ref_m) <= d_m, (c.name, k, mean[k - 1], ref_m, d_m)
                dv = v - ref_m
                ref_v = float((dv * dv).sum()) / mm
                bound = (mm + 4) * EPS * ref_v + 2 * float(np.abs(dv).mean()) * (EPS * float(np.abs(v).max()) + d_m)
                assert abs(var[k - 1] - ref_v) <= bound, (c.name, k, var[k - 1], ref_v, bound)
                assert std[k - 1] == math.sqrt(var[k - 1]) and var[k - 1] >= 0.0
                assert abs(lo[k - 1] - float(v.min())) <= EPS * abs(float(v.min())) and abs(hi[k - 1] - float(v.max())) <= EPS * abs(float(v.max()))
            faces = []
            for axis in (2, 1, 0):
                core = (slice(1, -1),) * 3
                faces.append(sum(float(((np.roll(padded, s, axis=axis)[core] != labels) & sel).sum()) for s in (1, -1)))
            ref_a = faces[0] * sp[1] * sp[2] + faces[1] * sp[0] * sp[2] + faces[2] * sp[0] * sp[1]
            assert abs(area[k - 1] - ref_a) <= 4 * EPS * ref_a and vol_[k - 1] == n * sp[0] * sp[1] * sp[2]
            assert abs(m.equivalent_diameter(sp)[k - 1] - (6.0 * vol_[k - 1] / math.pi) ** (1.0 / 3.0)) <= 4 * EPS * m.equivalent_diameter(sp)[k - 1]
            d = tuple(reversed(c.vol.shape))
            assert bool(m.touches_border[k - 1]) == bool((x.min() == 0) or (y.min() == 0) or (z.min() == 0) or (x.max() == d[0] - 1) or (y.max() == d[1] - 1) or (z.max() == d[2] - 1))
            assert np.array_equal(m.centroid_unit[k - 1], (cen[k - 1] + 0.5) / np.array(d, np.float64))
            checked += 1
    assert checked > 150


def test_a_ball_of_radius_10_in_32_cubed(libs, tmp_path):
    """The ball {|p - (16, 16, 16)|^2 <= 100} is centred on a voxel and has the cube's symmetries: its centroid is the centre, its covariance
    is a multiple of the identity and its faces are equal on the three axes, all exactly -- the spread of the principal lengths the float64
    reference gives over the ball's voxels is 0 up to eigh's rounding (asserted below 1e-12 of the length).  What the discretisation does
    show is the length itself: 2 sqrt(5 var) of these 4169 voxels against the continuous ball's 20."""
    z, y, x = np.indices((32, 32, 32))
    ball = (x - 16) ** 2 + (y - 16) ** 2 + (z - 16) ** 2 <= 100
    vol = np.where(ball, 200, 0).astype(np.uint8)
    c = MC.Case("ball", "ball", vol, "u8", 0.5, math.inf, 6, None, None, None, 0)
    table, fg = MH.restate_case(libs[0], libs[1], c)
    assert len(table) == 1 and fg == int(ball.sum()) == 4169
    m = _measurements(c, table, fg)
    assert np.abs(m.centroid[0] - 16.0).max() <= 1e-12 and np.abs(m.centroid_unit[0] - 16.5 / 32).max() <= 1e-12
    pos = np.stack([a[ball].astype(np.float64) for a in (x, y, z)])
    ref_cov = np.cov(pos, bias=True)
    ref_len = 2.0 * np.sqrt(5.0 * np.linalg.eigvalsh(ref_cov)[::-1])
    lengths = m.principal_lengths()[0]
    assert (ref_len.max() - ref_len.min()) <= 1e-12 * ref_len.max()                 # the expected spread: none
    assert (lengths.max() - lengths.min()) <= 1e-12 * lengths.max() and np.abs(lengths - ref_len).max() <= 1e-12 * ref_len.max()
    assert abs(lengths[0] - 20.0) < 0.1 and lengths[0] != 20.0                      # the discretisation of this ball: 2 sqrt(5 var) = 19.97...
    assert int(m.faces[0, 0]) == int(m.faces[0, 1]) == int(m.faces[0, 2]) > 0
    assert m.mean[0] == 200 / 255 and m.std[0] == 0.0 and m.min[0] == m.max[0] == 200 / 255 and not m.touches_border[0]
    assert abs(m.equivalent_diameter()[0] - 20.0) < 0.1
    assert m.surface_area()[0] > 4.0 * math.pi * 100.0 * 1.4                        # the staircase overestimates a smooth surface: towards 1.5
    path = tmp_path / "ball.csv"
    m.to_csv(path)
    lines = path.read_text().splitlines()
    assert lines[0] == m.CSV_HEADER and len(lines) == 2 and lines[1].split(",")[:3] == ["1", "4169", str(int(table[0, 1]))] and len(lines[1].split(",")) == len(m.CSV_HEADER.split(","))


@pytest.fixture(scope="module")
def bonsai():
    import __graft_entry__ as g

    g.build_host()
    exe = os.path.join(ROOT, "vokselis_amd", "_lib", "bonsai")
    assert os.path.exists(exe)
    return exe


@pytest.mark.parametrize("args, message", [
    (["--measure"], "--measure needs a value range: --components LO HI, or --iso V for [V, inf)"),
    (["--measure", "out.csv"], "--measure needs a value range: --components LO HI, or --iso V for [V, inf)"),
    (["--measure", "out.csv", "--iso", "0.3", "--gpus", "2"], "--measure runs on one GPU"),
    (["--measure", "--components", "0.3", "inf", "--morph-spacing", "0", "1", "1"], "--morph-spacing SX SY SZ: integers of 1 .. 64"),
    (["--measure", "--iso", "0.3", "--morph-fill", "1", "0"], "--morph-fill needs --morph"),
])
def test_bonsai_refuses_bad_measure_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
