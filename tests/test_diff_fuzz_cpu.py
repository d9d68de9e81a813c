"""The two references of vk_steady_diffusion held together over the shared cases (tests/diff_cases.py): the C
restatement (tests/diff_restatement.c: raster loops per colour) and the numpy reference (tests/np_diff_reference.py: whole-array float32
operations on padded shifts) -- c, dense array and every result word, bit for bit; the converged cases against a float64 direct solve of
the same linear system; the fixed cases with their pinned integers.  The conditions on the case list are asserted on the restatement's
output, so the list cannot quietly degenerate.  The host side -- the C boundary, vk_diff.hpp under ASan + UBSan (tests/diff_fuzz.cpp, a
stand-alone program), the Python surface, the derived values, bonsai's argument handling -- needs no GPU either."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import diff_cases as DFC
import diff_helpers as DH

ROOT = DH.ROOT
R = DH.R
# The largest deviations of the restatement from the float64 direct solve over the converged cases of at most 3000 foreground voxels,
# as measured ("Checks"): the relative deviation of the flux (a constriction) and |c - c64| (the fixed set in blocks
# of 4 sweeps).  The tests assert 4 times each: where float32 stagnates varies with the sweep count at which a case happens to stop.
MEASURED_FLUX, MEASURED_C = 4.475e-4, 1.221e-4


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return DH.build_restatement(tmp_path_factory.mktemp("diff_fuzz_cpu"))


@pytest.fixture(scope="module")
def restated(lib):
    return {c.name: DH.restate_case(lib, c) for c in DFC.cases()}


def _dims(c):
    return tuple(reversed(c.vol.shape))


def _f(word):
    return float(np.uint32(int(word)).view(np.float32))


def test_case_list_covers_the_issue(restated):
    cases = DFC.cases()
    assert len({c.name for c in cases}) == len(cases) and 60 <= len(cases) <= 150, len(cases)
    assert max(c.vol.size for c in cases) <= DFC.MAX_VOXELS == 64000
    src = open(os.path.join(ROOT, "vokselis_amd", "csrc", "vk_label.hpp")).read()
    assert tuple(int(v) for v in re.search(r"kLabelTile = \{(\d+)u, (\d+)u, (\d+)u,", src).groups()) == DFC.TILE == (32, 16, 8)
    dims = {_dims(c) for c in cases}
    assert set(DFC.DIMS) | {DFC.BIG, (37, 21, 11), (12, 7, 3)} <= dims
    assert all(any(d[a] == 1 for d in dims) for a in range(3))                                                   # 1 on each axis in turn
    assert any(DFC.extent(c)[c.axis] == 1 and int(restated[c.name][2][R["n_foreground"]]) > 1 for c in cases)     # n_a == 1: every voxel on both faces
    assert any(all(n % t for n, t in zip(d, DFC.TILE)) for d in dims) and any(all(n % t == 0 for n, t in zip(d, DFC.TILE)) for d in dims)
    assert all(n > 2 * t for n, t in zip(DFC.BIG, DFC.TILE))                                                       # 3 x 3 x 3 tiles
    for kind in ("u8", "u16", "f16"):
        mine = [c for c in cases if c.kind == kind]
        text = " | ".join(c.name for c in mine)
        for word in ("empty,", "full,", "no voxel on the inlet", "nothing percolates", "a sealed pocket", "a lone voxel", "parallel slabs", "a constriction", "density 0.31", "density 0.6",
                     "density 0.9", ", box (", "clip box", "empty box", "uniform noise", "the fixed set", "the full block"):
            assert word in text, (kind, word)
        assert {c.axis for c in mine} == {0, 1, 2} and {c.spacing for c in mine} >= set(DFC.SPACINGS) == {(1, 1, 1), (1, 1, 3), (2, 1, 1), (1, 2, 3)}
        assert {c.omega for c in mine} >= {0.0, 0.8, 1.0, 1.9} and {c.check_every for c in mine} >= {1, 4, 32}
    special = [c for c in cases if "NaN, inf" in c.name]
    assert {(c.lo, c.hi) for c in special} >= {(-math.inf, math.inf), (math.inf, math.inf), (-math.inf, -math.inf), (0.0, 0.0)}
    for c in special:  # a NaN texel is never in the set, whatever the range
        assert not (np.isnan(c.vol.astype(np.float32)) & (restated[c.name][0].view(np.uint32) != 0x7FC00000)).any(), c.name
    # what the cases exercise, on the restatement's output
    by = {c.name: (c, restated[c.name]) for c in cases}

    def one(word, kind="u8", **where):
        return next((c, r) for c, r in by.values() if c.kind == kind and word in c.name and all(getattr(c, k) == v for k, v in where.items()))

    results = [(c, r[2]) for c, r in by.values()]
    assert sum(int(r[R["converged"]]) == 1 and int(r[R["sweeps"]]) > c.check_every for c, r in results) >= 12        # run to convergence, over more than one block
    assert sum(int(r[R["converged"]]) == 0 and int(r[R["sweeps"]]) == c.max_sweeps // c.check_every * c.check_every for c, r in results) >= 20   # ended by max_sweeps
    assert any(int(r[R["converged"]]) == 1 and int(r[R["sweeps"]]) == c.check_every and int(r[R["n_foreground"]]) > 0 for c, r in results)         # in the very first block
    c, r = one("empty,")
    assert not r[2][:3].any() and int(r[2][R["n_box"]]) == c.vol.size and int(r[2][R["converged"]]) == 1 and (r[0].view(np.uint32) == 0x7FC00000).all()
    assert not r[2][R["Fin_q"]] and not r[2][R["Fout_q"]] and not r[2][R["sum_c_q"]] and not r[1].any()
    c, r = one("full,", axis=2)
    assert int(r[2][R["n_foreground"]]) == c.vol.size and int(r[2][R["n_inlet"]]) == int(r[2][R["n_outlet"]]) == 37 * 21 and int(r[2][R["converged"]]) == 1
    c, r = one("no voxel on the inlet")
    assert int(r[2][R["n_inlet"]]) == 0 and int(r[2][R["Fin_q"]]) == 0 and int(r[2][R["n_outlet"]]) > 0 and int(r[2][R["Fout_q"]]) > 0 and float(np.nanmax(r[0])) <= 0.5
    c, r = one("nothing percolates")
    assert int(r[2][R["converged"]]) == 1 and int(r[2][R["Fin_q"]]) == 0 == int(r[2][R["Fout_q"]]) and DH.flux(r[2]) == 0.0 and DH.derived(c, r[2])[1] == 0.0   # flux 0: tau is inf
    assert float(r[0][:, :, :18].min()) >= 0.999 and float(np.nanmax(r[0][:, :, 19:])) <= 1e-3                         # one block settles at the inlet's 1, the other at the outlet's 0
    c, r = one("a sealed pocket")
    pocket = DFC.pocket_mask(_dims(c))
    assert int(r[2][R["converged"]]) == 1 and pocket.sum() > 100 and float(np.abs(r[0][pocket] - 0.5).max()) <= 1e-6 and DH.flux(r[2]) > 1.0
    c, r = one("a lone voxel")
    assert int(r[2][R["n_foreground"]]) == 1 and float(np.nanmax(r[0])) == 0.5 and int(r[2][R["sum_c_q"]]) == 1 << 29 and _f(r[2][R["delta"]]) == 0.0 and int(r[2][R["converged"]]) == 1
    assert int(r[2][R["sweeps"]]) == c.check_every
    c, r = one("a constriction")
    assert int(r[2][R["converged"]]) == 1 and 0.0 < DH.derived(c, r[2])[1] < 0.2 * DH.derived(c, r[2])[0]              # the hole throttles the flux far below the porosity
    c, r = one("empty box")
    assert not r[2][:7].any() and int(r[2][R["converged"]]) == 1 and _f(r[2][R["omega"]]) == float(np.float32(2.0 / (1.0 + 3.141592653589793)))
    c, r = one("clip box")
    assert 0 < int(r[2][R["n_box"]]) < c.vol.size and c.clip is not None and c.box is not None
    c, r = one(", box (")
    assert int(r[2][R["n_box"]]) == 45 * 28 * 13 and (r[0].view(np.uint32)[:2] == 0x7FC00000).all()
    assert {_f(r[R["gain"]]) for _, r in results} >= {1.0, 0.5, 0.75, 2.0}
    for c, r in results:
        assert _f(r[R["omega"]]) == DFC.omega_used(c) and 0.0 < _f(r[R["omega"]]) < 2.0


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(restated):
    for c in DFC.cases():
        assert DH.differences(restated[c.name], DH.reference_case(c)) == "", c.name


def test_converged_cases_agree_with_a_float64_direct_solve(restated):
    """The physics: the float32 iteration against numpy.linalg.solve on the same system in float64.  The bounds are 4 times what was measured
    on the restatement (MEASURED_FLUX, MEASURED_C); that the measured flux deviation lies below flux_tol is a condition, not a measurement."""
    assert MEASURED_FLUX < 1e-3
    checked, worst_flux, worst_c = 0, 0.0, 0.0
    for c in DFC.cases():
        got_c, _, r = restated[c.name]
        if not int(r[R["converged"]]) or not 0 < int(r[R["n_foreground"]]) <= 3000:
            continue
        c64, fin, fout = DH.direct_solve(c)
        f64, f32 = 0.5 * (fin + fout), DH.flux(r)
        assert abs(fin - fout) <= 1e-9 * max(1.0, f64), c.name  # what goes in comes out
        rel = abs(f32 - f64) / f64 if f64 > 1e-12 else abs(f32 - f64)
        has = ~np.isnan(c64)
        dc = float(np.abs(got_c.astype(np.float64)[has] - c64[has]).max()) if has.any() else 0.0
        print(f"{c.name}: flux {f32:.9g}, float64 {f64:.9g}, relative {rel:.3e}, max |c - c64| {dc:.3e}")
        worst_flux, worst_c, checked = max(worst_flux, rel), max(worst_c, dc), checked + 1
        assert rel <= 4.0 * MEASURED_FLUX and dc <= 4.0 * MEASURED_C, (c.name, rel, dc)
    print(f"{checked} cases: worst relative flux deviation {worst_flux:.4e}, worst |c - c64| {worst_c:.4e}")
    assert checked >= 12 and worst_flux < 1e-3


def test_the_fixed_cases_give_the_pinned_numbers(lib, restated):
    tol = 4.0 * MEASURED_FLUX
    # the full 12 x 7 x 3 block along x: a straight channel, D_eff / D0 = 1, flux 21 / 12
    c = next(c for c in DFC.cases() if c.kind == "u8" and "the full block" in c.name)
    r = restated[c.name][2]
    porosity, deff = DH.derived(c, r)
    assert porosity == 1.0 and abs(deff - 1.0) <= tol and abs(DH.flux(r) - 1.75) <= 1.75 * tol and int(r[R["converged"]]) == 1
    # parallel slabs: D_eff / D0 is the porosity, along either open axis
    for c in (c for c in DFC.cases() if c.kind == "u8" and "parallel slabs" in c.name):
        porosity, deff = DH.derived(c, restated[c.name][2])
        assert porosity == 0.5 and abs(deff - porosity) <= porosity * tol, (c.name, deff)
    # the fixed mask of the geodesic cases along x, at the defaults: both references, every format
    pinned = dict(n_foreground=206, n_inlet=21, n_outlet=21, n_box=252, sweeps=96, converged=1, Fin_q=328591872, Fout_q=328737975, sum_c_q=101749242837)
    for c in (c for c in DFC.cases() if "the fixed set" in c.name and c.check_every == 32):
        for got in (restated[c.name], DH.reference_case(c)):
            assert {k: DH.signed(got[2][R[k]]) for k in pinned} == pinned, c.name
            assert int(got[2][R["delta"]]) == 0x36a40000 and int(got[2][R["omega"]]) == 0x3fce2cea and int(got[2][R["gain"]]) == 0x3f800000


def test_diffusion_derived_values_on_the_fixed_case(restated):
    import vokselis_amd as V

    c = next(c for c in DFC.cases() if c.kind == "u8" and "the fixed set" in c.name and c.check_every == 32)
    got_c, dense, r = restated[c.name]
    res = V.VkDiffusionResult(*[DH.signed(v) for v in r[:9]], _f(r[9]), _f(r[10]), _f(r[11]), 0)
    t = V.Diffusion(res, "x", (12, 7, 3), got_c, dense)
    assert (t.n_foreground, t.n_inlet, t.n_outlet, t.n_box, t.sweeps, t.converged, t.Fin_q, t.Fout_q, t.sum_c_q) == (206, 21, 21, 252, 96, True, 328591872, 328737975, 101749242837)
    assert t.flux_in == 328591872 / 2 ** 30 and t.flux_out == 328737975 / 2 ** 30 and t.flux == (328591872 + 328737975) / 2 ** 31
    assert t.flux_mismatch == (328737975 - 328591872) / (0.5 * (328591872 + 328737975)) < 1e-3
    assert t.porosity == 206 / 252 and t.effective_diffusivity == t.flux * 12 / 21 and t.tortuosity_factor == t.porosity / t.effective_diffusivity > 1.0
    assert t.mean_concentration == 101749242837 / (2 ** 30 * 206) and abs(t.mean_concentration - 0.46) < 0.05
    assert t.omega == float(np.float32(2.0 / (1.0 + 3.141592653589793 / 13.0))) and t.gain == 1.0 and t.delta == _f(0x36a40000) and t.axis == 0 and t.c is got_c and t.dense is dense
    nothing = V.Diffusion(V.VkDiffusionResult(10, 0, 5, 20, 0, 0, 5 << 30, 32, 1, 0.0, 1.5, 1.0, 0), 2, (5, 2, 2))
    assert (nothing.flux, nothing.effective_diffusivity, nothing.tortuosity_factor, nothing.flux_mismatch, nothing.porosity, nothing.mean_concentration) == (0.0, 0.0, math.inf, 0.0, 0.5, 0.5)
    empty = V.Diffusion(V.VkDiffusionResult(0, 0, 0, 0, 0, 0, 0, 32, 1, 0.0, 1.5, 1.0, 0), "y", (0, 2, 2))
    assert (empty.porosity, empty.mean_concentration, empty.tortuosity_factor, empty.effective_diffusivity) == (0.0, 0.0, math.inf, 0.0)


# ---- the C boundary -------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    for name, value in (("VK_DIFF_OFF", "0x7FC00000u"), ("VK_DIFF_MAX_CHECK_EVERY", "1024")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    assert "enum { VK_DIFF_CLIP_BOX = 1, VK_DIFF_INSTALL = 2 };" in code
    assert re.search(r"int vk_steady_diffusion\(vk_ctx \*ctx, const vk_diffusion_request \*req, const vk_voxel_box \*box, float \*c_out, void \*dense_out,\s*"
                     r"vk_diffusion_result \*result\);", code)
    assert "static_assert(sizeof(vk_diffusion_request) == 56 && sizeof(vk_diffusion_result) == 80" in code
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 32\. ", design, flags=re.M)
    section = design[design.index("## 32. "):]
    for phrase in ("3.141592653589793", "VK_DIFF_INSTALL", "1073741824"):
        assert phrase in _header(), phrase
        assert phrase in section, phrase
    for phrase in ("touch neither face", "x-, x+, y-, y+, z-, z+", "the product rounds, then the sum", "flux * n_a / (n_b * n_c)", "a NaN", "in this order"):
        assert phrase in _header(), phrase
    for word in ("The rule", "Structure", "Determinism", "Loop bounds", "Resources", "Measurements", "Checks", "Hosts", "Out of scope", "%.3e" % MEASURED_FLUX, "%.3e" % MEASURED_C):
        assert word in section, word
    assert "vk_steady_diffusion" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "steady_diffusion" in open(os.path.join(ROOT, "README.md")).read() and "--diffusion" in open(os.path.join(ROOT, "README.md")).read()
    assert "diff_quick.py" in open(os.path.join(ROOT, "tools", "README.md")).read() and os.path.exists(os.path.join(ROOT, "tools", "diff_quick.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "diff_pass_isa.txt"))


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_diff.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(vk_diffusion_request), offsetof(vk_diffusion_request, axis), '
                   'offsetof(vk_diffusion_request, spacing), offsetof(vk_diffusion_request, omega), offsetof(vk_diffusion_request, check_every), offsetof(vk_diffusion_request, max_sweeps), '
                   'offsetof(vk_diffusion_request, delta_tol), offsetof(vk_diffusion_request, gain), offsetof(vk_diffusion_request, fill_out), sizeof(vk_diffusion_result), '
                   'offsetof(vk_diffusion_result, n_box), offsetof(vk_diffusion_result, Fin_q), offsetof(vk_diffusion_result, sum_c_q), offsetof(vk_diffusion_result, sweeps), '
                   'offsetof(vk_diffusion_result, delta), VK_ABI_VERSION, VK_DIFF_MAX_CHECK_EVERY, VK_DIFF_INSTALL); return 0; }\n')
    exe = tmp_path / "sizeof_diff"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["56", "8", "16", "28", "32", "36", "40", "48", "52", "80", "24", "32", "48", "56", "64", "5", "1024", "2"], out


def test_the_binding_matches_and_every_export_resolves(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert (C.sizeof(N.VkDiffusionRequest), C.sizeof(N.VkDiffusionResult)) == (56, 80)
    assert [f[0] for f in N.VkDiffusionRequest._fields_] == ["lo", "hi", "axis", "flags", "spacing", "omega", "check_every", "max_sweeps", "delta_tol", "flux_tol", "gain", "fill_out"]
    assert [f[0] for f in N.VkDiffusionResult._fields_] == ["n_foreground", "n_inlet", "n_outlet", "n_box", "Fin_q", "Fout_q", "sum_c_q", "sweeps", "converged", "delta", "omega", "gain", "pad"]
    assert (N.VkDiffusionRequest.spacing.offset, N.VkDiffusionRequest.omega.offset, N.VkDiffusionRequest.gain.offset, N.VkDiffusionResult.Fin_q.offset, N.VkDiffusionResult.sweeps.offset,
            N.VkDiffusionResult.delta.offset) == (16, 28, 48, 32, 56, 64)
    declared = set(re.findall(r"\b(vk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)))
    assert "vk_steady_diffusion" in declared and declared == set(N.SYMBOLS), declared ^ set(N.SYMBOLS)
    assert hip_built.vk_steady_diffusion is not None
    # a NULL context: an error, the outputs untouched
    req, res, c = N.VkDiffusionRequest(), DH.fresh_result(N), np.full(8, 9, np.float32)
    assert hip_built.vk_steady_diffusion(None, C.byref(req), None, c.ctypes.data, None, C.byref(res)) == -1
    assert (c == 9).all() and res.n_foreground == 7 and res.sweeps == 7 and res.omega == 7.0


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context
    from vokselis_amd.diffusion import auto_omega, diffusion_request

    assert (V.DIFF_OFF, V.DIFF_MAX_CHECK_EVERY, V.DIFF_CLIP_BOX, V.DIFF_INSTALL) == (0x7FC00000, 1024, 1, 2)
    for name in ("DIFF_OFF", "DIFF_MAX_CHECK_EVERY", "DIFF_CLIP_BOX", "DIFF_INSTALL", "VkDiffusionRequest", "VkDiffusionResult", "Diffusion", "diffusion_request"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.steady_diffusion)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("lo", inspect.Parameter.empty), ("hi", math.inf), ("axis", "z"), ("spacing", (1, 1, 1)), ("omega", 0.0),
                                                                                ("check_every", 32), ("delta_tol", 1e-5), ("flux_tol", 1e-3), ("max_sweeps", 20000), ("gain", 0.0),
                                                                                ("fill_out", 0.0), ("box", None), ("install", False), ("out", False), ("c", False)]
    r = diffusion_request(0.3)
    assert (r.lo, r.hi, r.axis, r.flags, list(r.spacing), r.omega, r.check_every, r.max_sweeps, r.delta_tol, r.flux_tol, r.gain, r.fill_out) == \
        (np.float32(0.3), math.inf, 2, 0, [1, 1, 1], 0.0, 32, 20000, np.float32(1e-5), np.float32(1e-3), 0.0, 0.0)
    r = diffusion_request(0.2, 0.4, axis="x", spacing=(1, 2, 3), omega=1.5, check_every=8, delta_tol=0.0, flux_tol=0.5, max_sweeps=8, gain=0.25, fill_out=-0.5, box="clip", install=True)
    assert (r.axis, r.flags, list(r.spacing), r.omega, r.check_every, r.max_sweeps, r.delta_tol, r.flux_tol, r.gain, r.fill_out) == (0, 3, [1, 2, 3], 1.5, 8, 8, 0.0, 0.5, 0.25, -0.5)
    assert diffusion_request(0.2, axis=1).axis == 1 and diffusion_request(0.2, axis="y").axis == 1
    assert float(np.float32(auto_omega(12))) == DFC.auto_omega(12)
    for bad in (dict(spacing=(1, 1)), dict(spacing=(0, 1, 1)), dict(spacing=(1, 65, 1)), dict(spacing=(1.5, 1, 1)), dict(axis="w"), dict(axis=3), dict(axis=-1), dict(omega=2.0),
                dict(omega=-0.1), dict(omega=math.nan), dict(check_every=0), dict(check_every=1025), dict(check_every=1.5), dict(max_sweeps=31), dict(max_sweeps=2 ** 32),
                dict(delta_tol=-1.0), dict(delta_tol=math.inf), dict(flux_tol=math.nan), dict(gain=math.inf), dict(fill_out=math.nan)):
        with pytest.raises(ValueError):
            diffusion_request(0.3, **bad)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("diff_fuzz") / "diff_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "diff_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261021"])
def test_validation_order_q_the_update_and_the_replayed_blocks_under_sanitizers(fuzz_exe, seed):
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


NEEDS_RANGE = "--diffusion needs a value range: --components LO HI, or --iso V for [V, inf)"
AN_AXIS = "--diffusion AXIS [MAX_SWEEPS]: AXIS is x, y or z"
SWEEPS = "--diffusion AXIS [MAX_SWEEPS]: MAX_SWEEPS is an integer >= 32"


@pytest.mark.parametrize("args, message", [
    (["--diffusion", "x"], NEEDS_RANGE), (["--diffusion", "z", "500", "--morph-spacing", "1", "1", "2"], NEEDS_RANGE),
    (["--diffusion", "w", "--iso", "0.3"], AN_AXIS), (["--diffusion", "X", "--iso", "0.3"], AN_AXIS), (["--diffusion", "0", "--iso", "0.3"], AN_AXIS),
    (["--diffusion"], "missing value for --diffusion"),
    (["--iso", "0.3", "--diffusion", "x", "31"], SWEEPS), (["--iso", "0.3", "--diffusion", "x", "many"], SWEEPS), (["--iso", "0.3", "--diffusion", "x", "-5"], SWEEPS),
    (["--iso", "0.3", "--diffusion", "x", "--diffusion", "y"], "--diffusion: at most once"),
    (["--iso", "0.3", "--diffusion-install"], "--diffusion-install needs --diffusion AXIS"),
    (["--diffusion", "x", "--iso", "0.3", "--gpus", "2"], "--diffusion runs on one GPU"),
    (["--label-fill", "0.5", "--iso", "0.3", "--diffusion", "x"], "--label-fill needs a flag that drops voxels"),
])
def test_bonsai_refuses_bad_diffusion_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
