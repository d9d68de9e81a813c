"""The two references of vk_volume_filter held together over the shared cases (tests/filter_cases.py): the C
restatement (tests/filter_restatement.c: the rule's operations in order, -ffp-contract=off, an explicit fmaf) and the numpy reference
(tests/np_filter_reference.py: whole-array np.float32 operations, the fmaf by rounding to odd in float64) -- voxel for voxel, bit for bit.
The conditions on the case list are asserted on the restatement's counters and on the kernels' tile shapes, so the list cannot quietly
degenerate.  The properties of the rule are asserted on the restatement's output; the host side -- the C boundary, the Gaussian weights,
vk_filter.hpp under ASan + UBSan (tests/filter_fuzz.cpp, a stand-alone program), the Python surface -- needs no GPU either."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import filter_cases as FC
import filter_helpers as FH
import np_filter_reference as NF

ROOT = FH.ROOT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return FH.build_restatement(tmp_path_factory.mktemp("filter_fuzz_cpu"))


def test_case_list_covers_the_issue(lib):
    cases = FC.cases()
    assert len({c.name for c in cases}) == len(cases) and 100 <= len(cases) <= 260, len(cases)
    assert max(c.vol.size for c in cases) <= FC.MAX_VOXELS
    assert {tuple(reversed(c.vol.shape)) for c in cases} == set(FC.DIMS)
    assert FH.tile_shapes_in_the_header() == (FC.TILES, FC.MEDIAN_TILE)
    # the dimensions against the tile shapes, per axis
    for axis in range(3):
        dims = {d[axis] for d in FC.DIMS}
        edges = {t[axis] for t in FC.TILES} | {FC.MEDIAN_TILE[axis]}
        assert 1 in dims
        assert any(1 < n <= NF.MAX_RADIUS for n in dims)  # below radius + 1: the whole axis lies inside one halo
        for e in edges:
            assert e in dims and e + 1 in dims, (axis, e)
        assert any(n >= 2 * max(edges) + 1 and n % max(edges) for n in dims), axis
        assert any(n % 2 == 1 and n > 1 for n in dims)
    # the data and the filters, per format
    for kind in ("u8", "u16", "f16"):
        data = " | ".join(c.vol_id for c in cases if c.kind == kind)
        for word in ("constant", "two-valued", "uniform", "ball", "lone speckles", "saturating"):
            assert word in data, (kind, word)
        assert {c.name[len(c.vol_id) + 2:] for c in cases if c.kind == kind} == {f[0] for f in FC.FILTERS}, kind  # every filter on every format
    assert any("NaN, inf, -0, denormals" in c.name for c in cases) and any("denormals only" in c.name for c in cases)
    for name in FC.EVERY_DIMS:  # every dimension under the identity, the maximum radius and the median
        assert {tuple(reversed(c.vol.shape)) for c in cases if c.name.endswith(name)} == set(FC.DIMS), name
    # the radii: 0 on one, two and all axes; every class of tile
    zero_axes = {sum(1 for r in c.radii if r == 0) for c in cases if c.op == "convolve"}
    assert zero_axes == {0, 1, 2, 3}
    assert {max(c.radii) for c in cases if c.op == "convolve"} >= {0, 1, 2, 4, 5, 6}
    # what the cases exercise, on the restatement's counters
    total = np.zeros(len(FH.KINDS), np.uint64)
    per_kind = {k: np.zeros(len(FH.KINDS), np.uint64) for k in ("u8", "u16", "f16")}
    for c in cases:
        k = np.zeros(len(FH.KINDS), np.uint64)
        FH.restate_case(lib, c, k)
        total += k
        per_kind[c.kind] += k
    print("\nfilter cases: %d; %s" % (len(cases), ", ".join(f"{n} {int(v)}" for n, v in zip(FH.KINDS, total))))
    assert (total[:6] > 0).all(), total[:6]        # clamped taps on each side of each axis
    for kind in ("u8", "u16"):
        assert per_kind[kind][6] > 0 and per_kind[kind][7] > 0 and per_kind[kind][8] > 0, (kind, per_kind[kind])  # rint ties, clamped low and high
    assert per_kind["f16"][9] > 0 and per_kind["f16"][10] > 0   # NaN and infinite outputs
    assert all(per_kind[k][11] > 0 for k in per_kind)            # median ties


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(lib):
    for c in FC.cases():
        got = FH.restate_case(lib, c)
        ref = NF.apply(c.vol, c.kind, c.op, c.radii, c.weights)
        assert FH.differences(got, ref) == "", c.name


def test_all_radii_zero_is_the_identity(lib):
    n = 0
    for c in FC.cases():
        if c.op == "convolve" and max(c.radii) == 0:
            assert FH.same_bits(FH.restate_case(lib, c), NF.canonical(c.vol)), c.name
            n += 1
    assert n >= 3 * len(FC.DIMS) // 3
    # weights of a skipped axis are not read: NaNs there change nothing
    vol = np.random.default_rng(1).integers(0, 256, (5, 6, 7)).astype(np.uint8)
    junk = np.full(13, np.nan, np.float32)
    assert FH.same_bits(FH.restate(lib, vol, "u8", "convolve", (0, 0, 0), (junk, junk, junk)), vol)


@pytest.mark.parametrize("kind, value", [("u8", 77), ("u16", 40001), ("f16", 0.333), ("f16", -6e-8), ("u8", 255), ("u16", 0)])
def test_constant_volume_under_dyadic_weights_stays_constant(lib, kind, value):
    for d in ((9, 5, 5), (33, 9, 10), (1, 1, 1)):
        vol = np.full(FC.shape(d), value, NF.DTYPE[kind])
        for w in ((FC.DYADIC, FC.DYADIC, FC.DYADIC), (FC.DYADIC5, None, FC.DYADIC5), (None, FC.DYADIC, None)):
            radii = tuple(0 if x is None else len(x) // 2 for x in w)
            assert FH.same_bits(FH.restate(lib, vol, kind, "convolve", radii, w), vol), (d, radii)
        assert FH.same_bits(FH.restate(lib, vol, kind, "median3", (0, 0, 0), None), vol), d  # a fixed point of the median


@pytest.mark.parametrize("kind", ["u8", "u16", "f16"])
def test_lone_speckle_vanishes_under_the_median(lib, kind):
    for d, at in (((9, 5, 5), (2, 2, 4)), ((9, 5, 5), (0, 0, 0)), ((33, 9, 10), (9, 8, 32)), ((37, 5, 1), (0, 2, 17))):
        vol = np.zeros(FC.shape(d), NF.DTYPE[kind])
        vol[at] = NF.DTYPE[kind](1.0 if kind == "f16" else 200)
        out = FH.restate(lib, vol, kind, "median3", (0, 0, 0), None)
        assert not FH.raw(out).any(), (d, at)  # also in a corner (8 of the 27 clamped taps) and in a volume one voxel thick (3 of 27)


def test_median_output_is_one_of_its_27_inputs(lib):
    for c in FC.cases():
        if c.op != "median3":
            continue
        out = FH.restate_case(lib, c)
        hood = NF.neighbourhood(FH.raw(c.vol))
        assert (hood == FH.raw(out)[None]).any(axis=0).all(), c.name
        # and it is the 14th smallest: 13 at most below it, 13 at most above it, by the key
        keys = NF.key16(hood) if c.kind == "f16" else hood
        m = NF.key16(FH.raw(out)) if c.kind == "f16" else FH.raw(out)
        assert ((keys < m[None]).sum(axis=0) <= 13).all() and ((keys > m[None]).sum(axis=0) <= 13).all(), c.name


def test_integer_gaussian_is_within_one_lsb_of_a_float64_convolution(lib):
    n = 0
    for c in FC.cases():
        if c.kind == "f16" or "Gaussian" not in c.name:
            continue
        got = FH.restate_case(lib, c).astype(np.float64)
        exact = np.clip(NF.convolve_f64(c.vol, c.radii, c.weights), 0.0, NF.TOP[c.kind])
        assert np.abs(got - exact).max() <= 1.0, (c.name, float(np.abs(got - exact).max()))
        n += 1
    assert n >= 10


# ---- vk_filter_gaussian and the C boundary -------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_exports_and_the_struct_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert re.search(r"#define\s+VK_FILTER_MAX_RADIUS\s+6\b", code) and re.search(r"#define\s+VK_FILTER_MAX_WEIGHT\s+1024\.0f", code)
    assert "enum { VK_FILTER_CONVOLVE = 0, VK_FILTER_MEDIAN3 = 1 };" in code and "enum { VK_FILTER_INSTALL = 1 };" in code
    assert re.search(r"struct vk_volume_filter \{\s*int32_t\s+op;\s*uint32_t\s+flags;\s*uint32_t\s+radius\[3\];\s*float\s+weights\[3\]\[2 \* VK_FILTER_MAX_RADIUS \+ 1\];\s*\};", code)
    assert "int vk_volume_filter(vk_ctx *ctx, const struct vk_volume_filter *f, void *dense_out);" in code
    assert re.search(r"int vk_filter_gaussian\(double sigma_voxels, uint32_t radius, float \*weights\s*\);", code)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 22\. ", design, flags=re.M) and "vk_volume_filter" in design
    for phrase in ("acc = fmaf(w[k], t(c(x - r + k, nx), y, z), acc)", "ties to even", "0x7E00", "14th smallest", "totalOrder", "VK_FILTER_INSTALL"):
        assert phrase in _header(), phrase
        assert phrase in design[design.index("## 22. "):], phrase
    assert "vk_volume_filter" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_sizeof_the_struct_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_filter.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(struct vk_volume_filter), offsetof(struct vk_volume_filter, op), '
                   'offsetof(struct vk_volume_filter, flags), offsetof(struct vk_volume_filter, radius), offsetof(struct vk_volume_filter, weights), '
                   'VK_ABI_VERSION, VK_FILTER_MAX_RADIUS, VK_FILTER_MEDIAN3, VK_FILTER_INSTALL); return 0; }\n')
    exe = tmp_path / "sizeof_filter"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["176", "0", "4", "8", "20", "5", "6", "1", "1"], out


def _ulp_distance(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def test_gaussian_weights_and_the_null_context_refusals(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert C.sizeof(N.VkVolumeFilter) == 176 and [f[0] for f in N.VkVolumeFilter._fields_] == ["op", "flags", "radius", "weights"]
    for sigma in (0.3, 0.5, 0.8, 1.0, 1.7, 2.0, 2.5, 4.0, 10.0):
        for r in range(1, 7):
            w = np.full(2 * r + 3, -7.0, np.float32)
            assert hip_built.vk_filter_gaussian(sigma, r, w[1:].ctypes.data_as(C.POINTER(C.c_float))) == 0
            assert w[0] == -7.0 and w[-1] == -7.0
            w = w[1:-1]
            assert (w.view(np.uint32) == w[::-1].view(np.uint32)).all(), (sigma, r)     # symmetric bit for bit
            ref = NF.gaussian(sigma, r)
            assert max(_ulp_distance(a, b) for a, b in zip(w, ref)) <= 1, (sigma, r)   # libm's exp is not pinned bit for bit
            assert abs(float(w.astype(np.float64).sum()) - 1.0) <= (2 * r + 1) * 2.0 ** -24, (sigma, r)
    w = np.full(13, -7.0, np.float32)
    p = w.ctypes.data_as(C.POINTER(C.c_float))
    for sigma, r in ((0.0, 2), (-1.0, 2), (math.nan, 2), (math.inf, 2), (1.0, 0), (1.0, 7), (1.0, 2 ** 31)):
        assert hip_built.vk_filter_gaussian(sigma, r, p) == -1 and (w == -7.0).all(), (sigma, r)
        assert b"vk_filter_gaussian" in hip_built.vk_last_error(None)
    assert hip_built.vk_filter_gaussian(1.0, 2, None) == -1
    # a NULL context: an error, the output untouched
    req = N.VkVolumeFilter()
    out = np.full(8, 9, np.uint8)
    assert hip_built.vk_volume_filter(None, C.byref(req), out.ctypes.data) == -1 and (out == 9).all()


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context
    from vokselis_amd.filter import filter_request

    assert (V.FILTER_MAX_RADIUS, V.FILTER_MAX_WEIGHT, V.FILTER_CONVOLVE, V.FILTER_MEDIAN3, V.FILTER_INSTALL) == (6, 1024.0, 0, 1, 1)
    for name in ("FILTER_MAX_RADIUS", "FILTER_MAX_WEIGHT", "FILTER_CONVOLVE", "FILTER_MEDIAN3", "FILTER_INSTALL", "VkVolumeFilter", "gaussian_weights"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.filter_volume)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("weights", None), ("op", "convolve"), ("install", True), ("out", False)]
    for m in (Context.filter_volume, Context.smooth_volume, Context.median_volume):
        assert "filter_volume" in m.__doc__ or "vk_volume_filter" in m.__doc__
    assert [p.name for p in inspect.signature(V.gaussian_weights).parameters.values()] == ["sigma", "radius"]
    req = filter_request((FC.DYADIC, None, FC.DYADIC5), "convolve", install=False)
    assert list(req.radius) == [1, 0, 2] and req.flags == 0 and req.op == 0 and list(req.weights[2])[:5] == list(FC.DYADIC5) and list(req.weights[1]) == [0.0] * 13
    assert filter_request(None, "median3").op == 1 and filter_request(None, "median3").flags == 1
    for bad in (dict(weights=(FC.DYADIC, None)), dict(weights=([1.0, 2.0], None, None)), dict(weights=([1.0], None, None)), dict(weights=(np.ones(15), None, None)), dict(op="mean")):
        with pytest.raises(ValueError):
            filter_request(**bad)


def test_gaussian_weights_default_radius(hip_built):
    import vokselis_amd as V

    assert len(V.gaussian_weights(0.2)) == 3 and len(V.gaussian_weights(1.0)) == 7 and len(V.gaussian_weights(1.5)) == 11 and len(V.gaussian_weights(5.0)) == 13
    assert (V.gaussian_weights(1.0, 3).view(np.uint32) == V.gaussian_weights(1.0).view(np.uint32)).all()
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError):
            V.gaussian_weights(bad)
    with pytest.raises(V.VokselisError):
        V.gaussian_weights(1.0, 7)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("filter_fuzz") / "filter_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "filter_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261020"])
def test_tiles_halo_grid_store_rule_median_and_validation_under_sanitizers(fuzz_exe, seed):
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
    (["--save-raw", "out.raw"], "--save-raw writes the filtered volume: it needs --median or --smooth"),
    (["--save-raw"], "missing value for --save-raw"),
    (["--smooth", "1", "1"], "missing value for --smooth"),
    (["--smooth", "0", "0", "0"], "at least one sigma above 0"),
    (["--smooth", "1", "-1", "1"], "finite and >= 0"),
    (["--smooth", "nan", "1", "1"], "finite and >= 0"),
    (["--smooth", "1", "inf", "1"], "finite and >= 0"),
    (["--median", "--gpus", "2"], "--median and --smooth run on one GPU"),
    (["--smooth", "1", "1", "1", "--gpus", "2"], "--median and --smooth run on one GPU"),
])
def test_bonsai_refuses_bad_filter_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
