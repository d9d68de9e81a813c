"""The two references of vk_volume_resample held together over the shared cases (tests/resample_cases.py): the C
restatement (tests/resample_restatement.c: plain loops, every index and weight recomputed per voxel, -ffp-contract=off) and the numpy
reference (tests/np_resample_reference.py: whole-array np.float32 operations, the fmaf by rounding to odd in float64) -- voxel for
voxel, bit for bit.  The properties of the rule are asserted on the restatement's output, against the float64 definition and, where it
imports, scipy.ndimage.zoom; the host side -- the C boundary, vk_resample.hpp under ASan + UBSan (tests/resample_fuzz.cpp, a stand-alone
program), the Python surface, bonsai's arguments -- needs no GPU either."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import np_resample_reference as NR
import resample_cases as RC
import resample_helpers as RH

ROOT = RH.ROOT


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return RH.build_restatement(tmp_path_factory.mktemp("resample_fuzz_cpu"))


@pytest.fixture(scope="module")
def expected(lib):
    out = {}
    for c in RC.cases():
        e = RH.restate_case(lib, c)
        if e is not None:
            e.setflags(write=False)
        out[c.name] = e
    return out


def _nb(c):
    return (c.box[3] - c.box[0], c.box[4] - c.box[1], c.box[5] - c.box[2])


def _dims(c):
    return (c.vol.shape[2], c.vol.shape[1], c.vol.shape[0])


def test_case_list_covers_the_issue():
    cases = RC.cases()
    assert len({c.name for c in cases}) == len(cases) and 200 <= len(cases) <= 400, len(cases)
    assert max(c.vol.size for c in cases) == RC.MAX_VOXELS == 70 ** 3
    for axis in range(3):
        assert {_dims(c)[axis] for c in cases} == set(RC.SRC), axis
        assert {c.dims[axis] for c in cases} >= set(RC.OUT), axis
    for n in (37, 70, 67, 130):
        assert n in RC.OUT + RC.SRC and n % 64 and n % 4, n  # no multiple of the wave or of the tile's edges (64 x 4); 64 is exactly one tile edge
    for kind in RC.KINDS:
        mine = [c for c in cases if c.kind == kind and c.refused is None]
        assert {c.mode for c in mine} == set(RC.MODES)
        assert {(c.out, c.window is not None, c.mode) for c in mine} >= {(o, w, m) for o in RC.KINDS for w in (False, True) for m in RC.MODES}, kind
        data = " | ".join(c.vol_id for c in mine)
        for word in ("noise", "ramp", "zero", "maximum", "labels"):
            assert word in data, (kind, word)
        names = " | ".join(c.name for c in mine)
        for word in ("whole box", "one voxel box", "touches x-", "touches x+", "touches y-", "touches y+", "touches z-", "touches z+", "clip box", "ratio 16 box", "(identity)"):
            assert word in names, (kind, word)
        ratios = [tuple((nb > n) - (nb < n) for nb, n in zip(_nb(c), c.dims)) for c in mine]
        assert (1, 1, 1) in ratios and (-1, -1, -1) in ratios and any(1 in r and -1 in r for r in ratios), kind
        assert any(c.mode == "area" and max(nb / n for nb, n in zip(_nb(c), c.dims)) == 16 for c in mine), kind
        assert any(c.refused == -5 and c.mode == "area" for c in cases if c.kind == kind), kind
        lsb = {"u8": 1.0 / 255.0, "u16": 1.0 / 65535.0, "f16": 2.0 ** -11}[kind]
        assert any(c.window and c.window[1] - c.window[0] < lsb for c in mine), kind          # narrower than one LSB of the source
        assert any(c.window and c.window[0] < 0.0 and c.window[1] > 1.0 for c in mine), kind  # clamps neither end of the source's range ...
        assert any(c.window and c.window[0] > 0.0 and c.window[1] < 1.0 for c in mine), kind  # ... clamps both
    edges = next(c.vol for c in cases if c.vol_id == "f16 edges (70, 37, 37)")
    bits = edges.view(np.uint16)
    assert np.isnan(edges).any() and (bits == 0x7c00).any() and (bits == 0xfc00).any() and (bits == 0x0001).any() and (bits == 0x7bff).any() and float(np.float16(65504)) == 65504.0
    for c in cases:
        assert (c.refused is not None) == NR.refused(_nb(c), c.dims, c.mode), c.name
        if c.clip is not None:
            assert c.box == RC.clip_voxel_box(c.clip[0], c.clip[1], _dims(c))


def test_restatement_agrees_with_the_numpy_reference_bit_for_bit(expected):
    n = 0
    for c in RC.cases():
        if c.refused is not None:
            assert expected[c.name] is None, c.name
            continue
        assert RH.differences(expected[c.name], NR.resample(c.vol, c.kind, c.box, c.mode, c.dims, c.out, c.window)) == "", c.name
        n += 1
    assert n > 250


def test_the_identity_returns_the_stored_volume_bit_for_bit(lib, expected):
    n = 0
    for c in RC.cases():
        if "(identity)" not in c.name:
            continue
        want = RH.raw(c.vol).copy()
        got = RH.raw(expected[c.name])
        if c.kind == "f16" and c.mode != "nearest":  # LINEAR and AREA go through the store rule: a NaN's payload becomes 0x7E00
            nan = np.isnan(c.vol)
            assert (got[nan] == 0x7e00).all(), c.name
            got, want = got[~nan], want[~nan]
        assert (got == want).all(), c.name
        n += 1
    assert n == 3 * 7
    for kind, d in (("u8", (5, 3, 2)), ("u16", (37, 2, 3)), ("f16", (1, 1, 70))):  # ... and with every dims of 0: the box's own extents
        vol = RC.noise(d, kind, 5)
        for mode in RC.MODES:
            assert RH.differences(RH.restate(lib, vol, kind, (0, 0, 0) + d, mode, d, kind, None), vol) == "", (kind, mode)


def test_resampling_a_box_is_resampling_an_upload_of_the_cropped_array(lib, expected):
    n = 0
    for c in RC.runnable():
        if c.box == (0, 0, 0) + _dims(c):
            continue
        sub = NR.crop(c.vol, c.box)
        alone = RH.restate(lib, sub, c.kind, (0, 0, 0) + _nb(c), c.mode, c.dims, c.out, c.window)
        assert RH.differences(expected[c.name], alone) == "", c.name
        n += 1
    assert n > 100


def test_nearest_outputs_are_a_subset_of_the_inputs(expected):
    n = 0
    for c in RC.runnable():
        if c.mode == "nearest" and c.out == c.kind and c.window is None:
            assert np.isin(RH.raw(expected[c.name]), RH.raw(NR.crop(c.vol, c.box))).all(), c.name
            n += 1
    assert n > 20


def test_area_by_2_3_and_4_on_integer_data_is_the_exact_block_mean_rounded_once(expected):
    n = 0
    for c in RC.runnable():
        if "blocks of" not in c.name or c.kind == "f16":
            continue
        sub = NR.crop(c.vol, c.box).astype(np.int64)
        f = tuple(nb // m for nb, m in zip(_nb(c), c.dims))
        assert all(m * k == nb for nb, m, k in zip(_nb(c), c.dims, f)), c.name
        s = sub.reshape(c.dims[2], f[2], c.dims[1], f[1], c.dims[0], f[0]).sum(axis=(1, 3, 5))
        count = f[0] * f[1] * f[2]
        q, r = s // count, s % count
        mean = q + ((2 * r > count) | ((2 * r == count) & (q % 2 == 1)))  # rounded once, ties to even
        assert (expected[c.name].astype(np.int64) == mean).all(), c.name
        n += 1
    assert n == 6


def test_area_of_a_constant_volume_is_that_constant_at_every_ratio(lib):
    worst = 0
    for kind, value in (("u8", 255), ("u8", 77), ("u16", 65535), ("u16", 40001), ("f16", 0.333), ("f16", 65504.0)):
        for nb in RC.SRC:
            for n in RC.OUT:
                if nb > RC.MAX_RATIO * n:
                    continue
                vol = np.full(RC.shape((nb, 3, 2)), value, RC.DTYPE[kind])
                got = RH.restate(lib, vol, kind, (0, 0, 0, nb, 3, 2), "area", (n, 2, 3), kind, None)
                worst = max(worst, int(np.abs(RH.raw(got).astype(np.int64) - int(RH.raw(vol)[0, 0, 0])).max()))
    assert worst == 0, worst


def _f32_error_bound(c):
    """An upper bound, in units of the output format's scale, of what f32 rounding moves the value before the store, from the rule alone.
    M is the largest |texel| of the box; every f32 rounding of a value of at most M moves it by at most 2^-24 M.  LINEAR rounds twice per
    lerp (the difference, the fma) and the fraction's own rounding moves the lerp by at most 2^-24 * 2 M; a level passes its inputs'
    errors on as a convex combination, three levels: K = 12.  AREA rounds once per tap, at most 17 per axis, and the weights' roundings
    add up to 2^-24 M per axis: K = 54.  The map multiplies all of it by a, adds the roundings of a (2^-24 a M), of b (2^-24 |b|) and
    of its own fma (2^-24 of the result, at most the format's top once clamped)."""
    m = float(np.abs(NR.crop(c.vol, c.box).astype(np.float64)).max())
    k = 12 if c.mode == "linear" else 54
    if c.out == c.kind and c.window is None:
        return k * m * 2.0 ** -24
    a, b = NR.value_map(c.kind, c.out, c.window, True)
    return (a * m * (k + 1) + abs(b) + max(a * m + abs(b), NR.SCALE[c.out])) * 2.0 ** -24


def test_integer_outputs_lie_within_one_lsb_of_the_float64_definition(expected):
    """Every case whose f32 error bound stays below 0.45 LSB of the output: the rounding of the store adds at most 0.5.  The cut is on
    the amplification itself, a M 2^-24 K: a window narrower than one LSB of a u16 source into u16 multiplies the interpolated
    value's rounding by tens of thousands and is left out, the window 0.4 .. 0.45 from u16 into u8 (a = 0.08) is not."""
    n = windows = 0
    worst = {"linear": 0.0, "area": 0.0}
    for c in RC.runnable():
        if c.mode == "nearest" or c.out == "f16" or c.vol_id.startswith("f16 edges"):
            continue
        bound = _f32_error_bound(c)
        if bound >= 0.45:
            continue
        exact = np.clip(NR.definition(c.vol, c.kind, c.box, c.mode, c.dims, c.out, c.window), 0.0, RC.TOP[c.out])
        err = float(np.abs(expected[c.name].astype(np.float64) - exact).max())
        if c.out == c.kind and c.window is None:
            worst[c.mode] = max(worst[c.mode], err)
        assert err < 1.0 and err <= 0.5 + bound, (c.name, err, bound)
        n += 1
        windows += c.window is not None
    print("\nresample: integer outputs against the float64 definition over %d cases (%d windowed), worst |difference| in LSB without a map: %s" % (n, windows, worst))
    assert n > 60 and windows > 15


def test_f16_outputs_are_the_definitions_nearest_half_or_a_neighbour(expected):
    """Voxel by voxel, wherever the f32 error bound is at most half the spacing of the halves at the exact value: there the rounded f32
    value is the exact value's nearest half or a neighbour of it.  Where terms cancel -- signed noise, a value at a window's lo -- the
    exact value is small, its halves are dense, and the voxel is left out; the edge volumes (infinities, NaN) have no bound."""
    n = checked = total = 0
    for c in RC.runnable():
        if c.mode == "nearest" or c.out != "f16" or c.vol_id.startswith("f16 edges"):
            continue
        bound = _f32_error_bound(c)
        exact = NR.definition(c.vol, c.kind, c.box, c.mode, c.dims, c.out, c.window)
        with np.errstate(over="ignore", invalid="ignore"):
            near = exact.astype(np.float16)
            up, down = np.nextafter(near, np.float16(np.inf)), np.nextafter(near, np.float16(-np.inf))
            spacing = np.minimum(up.astype(np.float64) - near.astype(np.float64), near.astype(np.float64) - down.astype(np.float64))
            held = np.isfinite(spacing) & (bound <= 0.5 * spacing)
            got = np.asarray(expected[c.name])
            ok = (got == near) | (got == up) | (got == down)
        assert ok[held].all(), (c.name, int((~ok[held]).sum()))
        n += 1
        checked += int(held.sum())
        total += held.size
    print("\nresample: R16F outputs against the float64 definition over %d cases, %d of %d voxels inside the bound" % (n, checked, total))
    assert n > 40 and checked > 0.9 * total


@pytest.mark.parametrize("kind, out", [(k, o) for k in RC.KINDS for o in ("u8", "u16")])
def test_a_windowed_conversion_of_a_ramp_is_monotone_and_hits_both_ends(lib, kind, out):
    n = 4097
    lo, hi = (0.25, 0.75)
    if kind == "f16":
        vol = np.linspace(0.0, 1.0, n).astype(np.float16).reshape(1, 1, n)
        at_lo, at_hi = np.float16(lo), np.float16(hi)
    else:
        top = RC.TOP[kind]
        vol = np.rint(np.linspace(0.0, top, n)).astype(RC.DTYPE[kind]).reshape(1, 1, n)
        # sample values the format holds exactly: the window's ends on stored texels
        k_lo, k_hi = top // 5, 4 * top // 5
        lo, hi = float(np.float32(k_lo / top)), float(np.float32(k_hi / top))
        vol[0, 0, 1], vol[0, 0, -2] = k_lo, k_hi
        vol = np.sort(vol, axis=2)
        at_lo, at_hi = k_lo, k_hi
    for mode in ("nearest", "linear"):
        got = RH.restate(lib, vol, kind, (0, 0, 0, n, 1, 1), mode, (n, 1, 1), out, (lo, hi))[0, 0].astype(np.int64)
        assert (np.diff(got) >= 0).all(), mode
        src = vol[0, 0]
        assert (got[src <= at_lo] == 0).all() and (got[src >= at_hi] == RC.TOP[out]).all() and got.min() == 0 and got.max() == RC.TOP[out], mode
        inside = (src > at_lo) & (src < at_hi)
        assert inside.any() and (got[inside] >= 0).all() and len(np.unique(got[inside])) > 50


def test_linear_definition_agrees_with_scipy_zoom():
    ndimage = pytest.importorskip("scipy.ndimage")
    n = 0
    worst = 0.0
    for c in RC.runnable():
        if c.mode != "linear" or c.kind == "f16" or c.out != c.kind or c.window is not None:
            continue
        sub = NR.crop(c.vol, c.box).astype(np.float64)
        zoom = tuple(m / nb for m, nb in zip(reversed(c.dims), sub.shape))
        if tuple(int(round(s * z)) for s, z in zip(sub.shape, zoom)) != tuple(reversed(c.dims)):
            continue
        ref = ndimage.zoom(sub, zoom, order=1, mode="nearest", grid_mode=True)
        if ref.shape != tuple(reversed(c.dims)):
            continue
        mine = NR.definition(c.vol, c.kind, c.box, c.mode, c.dims, c.out, c.window)
        err = float(np.abs(mine - ref).max() / max(1.0, np.abs(ref).max()))
        worst = max(worst, err)
        assert err <= 1e-6, (c.name, err)
        n += 1
    print("\nresample: float64 LINEAR definition against scipy.ndimage.zoom over %d cases, worst relative difference %.3g" % (n, worst))
    assert n >= 10


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()


def test_header_declares_the_export_and_the_structs_and_keeps_the_abi_number():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+VK_ABI_VERSION\s+5\b", code)
    assert re.search(r"#define\s+VK_RESAMPLE_KEEP_FORMAT\s+\(-1\)", code) and re.search(r"#define\s+VK_RESAMPLE_MAX_RATIO\s+16\b", code)
    assert "enum { VK_RESAMPLE_NEAREST = 0, VK_RESAMPLE_LINEAR = 1, VK_RESAMPLE_AREA = 2 };" in code
    assert "enum { VK_RESAMPLE_INSTALL = 1, VK_RESAMPLE_CLIP_BOX = 2, VK_RESAMPLE_WINDOW = 4 };" in code
    assert "int vk_volume_resample(vk_ctx *ctx, const vk_resample_request *req, const vk_voxel_box *box, void *dense_out, vk_resample_result *result);" in code
    assert "int vk_resample_output(vk_ctx *ctx, const vk_resample_request *req, const vk_voxel_box *box, vk_resample_result *result);" in code
    for phrase in ("floor((2 j + 1) nb / (2 n))", "(f == 0) ? a : fmaf(f, b - a, a)", "min((j + 1) nb, (k + 1) n) - max(j nb, k n)", "clamped to B, not to the volume",
                   "a = S_out / ((hi - lo) S_in)", "0x7E00", "ties to even", "unit-cube coordinates of the\n * NEW volume", "resample: "):
        assert phrase in _header(), phrase
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"^## 26\. ", design, flags=re.M) and "vk_volume_resample" in design[design.index("## 26. "):]
    assert "vk_volume_resample" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_sizeof_the_structs_from_a_compiled_c_snippet(tmp_path):
    src = tmp_path / "sizeof_resample.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "vokselis_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(vk_resample_request), offsetof(vk_resample_request, mode), '
                   'offsetof(vk_resample_request, flags), offsetof(vk_resample_request, dims), offsetof(vk_resample_request, format), offsetof(vk_resample_request, layout), '
                   'offsetof(vk_resample_request, lo), offsetof(vk_resample_request, hi), sizeof(vk_resample_result), offsetof(vk_resample_result, dims), '
                   'offsetof(vk_resample_result, format), offsetof(vk_resample_result, layout), offsetof(vk_resample_result, box), '
                   'VK_ABI_VERSION, VK_RESAMPLE_AREA, VK_RESAMPLE_WINDOW, VK_RESAMPLE_KEEP_FORMAT, VK_RESAMPLE_MAX_RATIO); return 0; }\n')
    exe = tmp_path / "sizeof_resample"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["36", "0", "4", "8", "20", "24", "28", "32", "44", "0", "12", "16", "20", "5", "2", "4", "-1", "16"], out


def test_the_ctypes_mirrors_and_a_null_context(hip_built):
    from vokselis_amd import _native as N

    assert hip_built.vk_abi_version() == 5
    assert C.sizeof(N.VkResampleRequest) == 36 and [f[0] for f in N.VkResampleRequest._fields_] == ["mode", "flags", "dims", "format", "layout", "lo", "hi"]
    assert C.sizeof(N.VkResampleResult) == 44 and [f[0] for f in N.VkResampleResult._fields_] == ["dims", "format", "layout", "box"]
    assert [getattr(N.VkResampleRequest, f).offset for f in ("mode", "flags", "dims", "format", "layout", "lo", "hi")] == [0, 4, 8, 20, 24, 28, 32]
    assert "vk_volume_resample" in N.SYMBOLS and "vk_resample_output" in N.SYMBOLS
    assert hip_built.vk_resample_output(None, C.byref(N.VkResampleRequest()), None, C.byref(N.VkResampleResult())) == -1
    req, res = N.VkResampleRequest(), N.VkResampleResult()
    out = np.full(8, 9, np.uint8)
    assert hip_built.vk_volume_resample(None, C.byref(req), None, out.ctypes.data, C.byref(res)) == -1 and (out == 9).all() and tuple(res.dims) == (0, 0, 0)


def test_python_surface():
    import vokselis_amd as V
    from vokselis_amd.context import Context

    assert (V.RESAMPLE_NEAREST, V.RESAMPLE_LINEAR, V.RESAMPLE_AREA, V.RESAMPLE_INSTALL, V.RESAMPLE_CLIP_BOX, V.RESAMPLE_WINDOW, V.RESAMPLE_KEEP_FORMAT, V.RESAMPLE_MAX_RATIO) == (0, 1, 2, 1, 2, 4, -1, 16)
    for name in ("RESAMPLE_NEAREST", "RESAMPLE_LINEAR", "RESAMPLE_AREA", "RESAMPLE_INSTALL", "RESAMPLE_CLIP_BOX", "RESAMPLE_WINDOW", "RESAMPLE_KEEP_FORMAT", "RESAMPLE_MAX_RATIO",
                 "VkResampleRequest", "VkResampleResult", "resample_request"):
        assert name in V.__all__ and hasattr(V, name), name
    sig = inspect.signature(Context.resample_volume)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("dims", None), ("scale", None), ("box", None), ("mode", "linear"), ("fmt", None), ("window", None),
                                                                               ("layout", None), ("install", True), ("out", False)]
    for m in (Context.resample_volume, Context.crop_volume, Context.downsample_volume, Context.isotropic_volume):
        assert "resample_volume" in m.__doc__ or "vk_volume_resample" in m.__doc__
    assert list(inspect.signature(Context.crop_volume).parameters)[1] == "box" and list(inspect.signature(Context.downsample_volume).parameters)[1] == "factor"
    assert [(p.name, p.default) for p in list(inspect.signature(Context.isotropic_volume).parameters.values())[1:3]] == [("spacing", inspect.Parameter.empty), ("mode", "linear")]


def test_resample_request_mirrors_the_refusals():
    import vokselis_amd as V
    from vokselis_amd.resample import downsample_dims, isotropic_dims, value_map

    r = V.resample_request((3, 0, None), "area", "u8", (0.1, 0.6), V.LAYOUT_PACKED, "clip", install=True, out=True)
    assert (r.mode, r.flags, tuple(r.dims), r.format, r.layout) == (2, 1 | 2 | 4, (3, 0, 0), V.FMT_R8_UNORM, V.LAYOUT_PACKED)
    assert r.lo == np.float32(0.1) and r.hi == np.float32(0.6)
    r = V.resample_request(install=False, out=True)
    assert (r.mode, r.flags, tuple(r.dims), r.format, r.layout) == (1, 0, (0, 0, 0), -1, 0)
    assert V.resample_request(fmt=V.FMT_R16_UNORM).format == 3 and V.resample_request(fmt="f16").format == 1
    for bad in (dict(mode="cubic"), dict(fmt="rgba"), dict(fmt=V.FMT_RGBA16F_PAIR), dict(fmt=7), dict(dims=(1, 2)), dict(dims=(1, 2, 65536)), dict(dims=(-1, 2, 3)),
                dict(window=(0.5, 0.5)), dict(window=(0.6, 0.5)), dict(window=(0.0, math.inf)), dict(window=(math.nan, 1.0)), dict(window=(0.0, 1e39)),
                dict(install=False, out=False), dict(layout=7), dict(layout=-1), dict(box="all"), dict(box=((0, 0), (1, 1)))):
        with pytest.raises(ValueError):
            V.resample_request(**bad)
    assert V.resample_request(dims=(65535, 1, 1)).dims[0] == 65535
    assert downsample_dims((70, 37, 5), 2) == (35, 19, 3) and downsample_dims((70, 37, 5), (1, 4, 16)) == (70, 10, 1)
    assert isotropic_dims((512, 512, 300), (1.0, 1.0, 2.0)) == (512, 512, 600) and isotropic_dims((10, 10, 1), (0.5, 1.0, 0.01)) == (500, 1000, 1)
    for bad in (0, 1.5, (2, 2), -1):
        with pytest.raises(ValueError):
            downsample_dims((4, 4, 4), bad)
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, math.inf, 1.0)):
        with pytest.raises(ValueError):
            isotropic_dims((4, 4, 4), bad)
    a, b = value_map(V.FMT_R16_UNORM, V.FMT_R8_UNORM, 0.25, 0.75)
    assert a == np.float32(255.0 / (0.5 * 65535.0)) and b == np.float32(-127.5)
    assert tuple(float(v) for v in NR.value_map("u16", "u8", (0.25, 0.75))) == (float(a), float(b))


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resample_fuzz") / "resample_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "resample_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261020"])
def test_geometry_tables_offsets_grid_and_validation_under_sanitizers(fuzz_exe, seed):
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
    (["--crop", "1", "2", "3", "4", "5"], "missing value for --crop"),
    (["--crop", "4", "0", "0", "4", "8", "8"], "a half-open box with X0 < X1"),
    (["--crop", "0", "0", "0", "70000", "8", "8"], "voxel indices of 0 .. 65535"),
    (["--crop", "-1", "0", "0", "4", "8", "8"], "voxel indices of 0 .. 65535"),
    (["--crop", "clip", "--histogram", "16"], "--crop clip needs --clip"),
    (["--resample", "8", "8"], "missing value for --resample"),
    (["--resample", "8", "8", "65536"], "extents of 0 .. 65535"),
    (["--resample", "8", "8", "8", "cubic"], "MODE is nearest, linear or area"),
    (["--downsample", "0"], "an integer of 1 .. 16"),
    (["--downsample", "17"], "an integer of 1 .. 16"),
    (["--isotropic", "1", "0", "1"], "finite spacings above 0"),
    (["--isotropic", "1", "nan", "1"], "finite spacings above 0"),
    (["--to-u8", "0.5", "0.5"], "finite sample values with LO < HI"),
    (["--to-u16", "0.1", "inf"], "finite sample values with LO < HI"),
    (["--to-u8", "0.1"], "missing value for --to-u8"),
    (["--downsample", "2", "--gpus", "2"], "run on one GPU"),
    (["--downsample", "2"] * 17, "at most 16 together"),
])
def test_bonsai_refuses_bad_resample_arguments_before_it_touches_a_device(bonsai, args, message):
    r = subprocess.run([bonsai] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and message in r.stderr, (args, r.returncode, r.stderr[-500:])
