"""R16_UNORM volumes on the CPU (VK_FMT_R16_UNORM): the numpy references on the u16 scale (tests/np_u16_reference.py)
among themselves over the shared cases (tests/u16_cases.py), the emptiness predicates under sanitizers (tests/u16_fuzz.cpp), and the Python
wrapper's fmt= rules.

1. Widening.  A u8 volume times 257 is the same volume on the u16 scale (v * 257 / 65535 = v / 255): for the widening cases the u16
   reference's step image equals the u8 reference's on every pixel and the colour agrees within 1e-5, in every family.
2. Coverage.  Every case steps on >= 2 % of its pixels, and every noisy case's frame differs from the frame of its high byte alone on >= 2 %
   of them: a decode that drops the low byte cannot pass the GPU comparison.
3. Predicate fuzz: u16_fuzz, a program of its own under ASan + UBSan.
4. The wrapper: fmt=FMT_R16_UNORM takes a 3-D uint16 array and nothing else; a bare uint16 array still uploads as f16 bit patterns."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import np_builtin_reference as NB
import np_iso_reference as NI
import np_mip_reference as NM
import np_table_reference as NT
import np_u16_reference as NU
import u16_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_abi_names_the_format():
    from vokselis_amd import _native as N

    assert N.FMT_R16_UNORM == 3 and (N.FMT_R8_UNORM, N.FMT_R16_FLOAT, N.FMT_RGBA16F_PAIR) == (0, 1, 2)
    hdr = open(os.path.join(ROOT, "include", "vokselis_hip.h")).read()
    assert "VK_FMT_R16_UNORM = 3" in hdr and "#define VK_ABI_VERSION 5" in hdr


def test_the_substitution_is_restored(O):
    saved = (NT.tf_constants, NM.tf_constants, NI.iso_k, NB.transfer_alpha, NB.tap_empty)
    with NU.u16():
        assert NT.tf_constants is NU.tf_constants and NB.tap_empty is NU.tap_empty
    assert (NT.tf_constants, NM.tf_constants, NI.iso_k, NB.transfer_alpha, NB.tap_empty) == saved
    # the split of the built-in transfer, over every tap value
    t = np.arange(65536, dtype=np.float32)
    assert ((NU.transfer_alpha(t) == 0) == (t <= 6553)).all() and (NU.tap_empty(t) == (t <= 6553)).all()


def test_widening_gives_the_u8_frames(O):
    """(1): steps equal on every pixel, colour within 1e-5."""
    wide = [c for c in u16_cases.cases(O) if c.u8 is not None]
    assert {c.family for c in wide} == set(u16_cases.FAMILIES)
    for c in wide:
        assert (c.vol == c.u8.astype(np.uint16) * 257).all()
        cam = O.camera_blob(*c.cam)
        rgb, steps, _ = u16_cases.reference(O, c)
        if c.family == "builtin":
            r8, s8, _ = NB.render(cam, c.u8, c.W, c.H, dt=c.dt)
        elif c.family in ("table", "lit"):
            r8, s8 = NT.render(cam, c.u8, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt, light=c.light if c.family == "lit" else None)
        elif c.family in ("mip", "mipgrey"):
            r8, s8, _ = NM.render(cam, c.u8, c.W, c.H, table=c.table, domain=c.domain, dt=c.dt)
        else:
            r8, s8 = NI.render(cam, c.u8, c.W, c.H, iso=c.iso, colour=c.colour, refine=c.refine, dt=c.dt, light=c.light)[:2]
        d = float(np.abs(rgb - r8).max())
        print(f"{c.name}: {int((steps != s8).sum())} steps differ, max |d colour| {d:.3g}")
        assert (steps == s8).all(), c
        assert d <= 1e-5, (c, d)


def test_every_case_steps_and_the_low_byte_shows(O):
    """(2)"""
    noisy = 0
    for c in u16_cases.cases(O):
        rgb, steps, _ = u16_cases.reference(O, c)
        px = c.W * c.H
        assert (steps > 0).sum() >= 0.02 * px, (c, int((steps > 0).sum()), px)
        assert np.isfinite(rgb).all(), c
        if c.family == "iso":  # an isosurface case shows its surface
            assert (rgb > 0).any(axis=2).sum() >= 0.02 * px, (c, int((rgb > 0).any(axis=2).sum()), px)
        if c.noisy:
            noisy += 1
            high, hsteps, _ = u16_cases.reference(O, c, vol=c.vol & np.uint16(0xFF00))
            differ = (np.abs(rgb - high) > 1e-4).any(axis=2) | (steps != hsteps)
            assert differ.sum() >= 0.02 * px, (c, int(differ.sum()), px)
    assert noisy >= 12 and sum(c.noisy and c.family == f for c in u16_cases.cases(O) for f in ("iso",)) >= 3
    assert all(sum(c.noisy and c.family == f for c in u16_cases.cases(O)) >= 1 for f in u16_cases.FAMILIES)
    assert {c.lit for c in u16_cases.cases(O) if c.family == "iso"} == {True, False}
    fams = {(c.family, c.box is not None) for c in u16_cases.cases(O)}
    assert {f for f, _ in fams} == set(u16_cases.FAMILIES) and {f for f, b in fams if b} >= {"table", "lit", "mip", "iso"}
    assert {c.refine for c in u16_cases.cases(O) if c.family == "iso"} == {0, 4, 16}
    assert sum(c.half for c in u16_cases.cases(O)) >= 4


def test_the_constants_census(O):
    """The built-in transfer's empty fractions of the constant volumes: 1, 1, 0, 0 for 0, 6553, 6554, 65535."""
    got = [(int(c.vol.flat[0]), NU.empty_fraction(c.vol), c.empty) for c in u16_cases.cases(O) if c.empty is not None]
    assert [(v, e) for v, e, _ in got] == [(0, 1.0), (6553, 1.0), (6554, 0.0), (65535, 0.0)] and all(e == w for _, e, w in got)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("u16_fuzz") / "u16_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "u16_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15"])
def test_empty_u16_cells_contribute_nothing_under_sanitizers(fuzz_exe, seed):
    """(3)"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "60000", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    bad = r.stdout.split("bad ")[1].split(" of ")[0]
    empties = [int(v) for v in r.stdout.split("(")[-1].split(" empty")[0].split()]
    assert bad == "0" and len(empties) == 4 and min(empties) > 1000, r.stdout  # (the fuzz must reach empty cells under every predicate)


class _FakeLib:
    """Records vk_volume_upload's arguments instead of uploading."""

    def __init__(self):
        self.calls = []

    def vk_volume_upload(self, ctx, p, p2, nx, ny, nz, fmt, layout):
        self.calls.append((nx, ny, nz, fmt, layout, bytes((ctypes.c_ubyte * 4).from_address(p))))
        return 0


def test_the_wrapper_fmt_rules(monkeypatch, tmp_path):
    """(4)"""
    import vokselis_amd as V
    from vokselis_amd import _native as N

    fake = _FakeLib()
    monkeypatch.setattr(N, "lib", lambda: fake)

    class Ctx:
        handle = None

    u16 = np.arange(2 * 3 * 4, dtype=np.uint16).reshape(2, 3, 4) + 0x3C00
    # a bare uint16 array still means f16 bit patterns; so does a float16 array
    assert V.VolumeTexture(Ctx, u16).format == V.FMT_R16_FLOAT and fake.calls[-1][:4] == (4, 3, 2, V.FMT_R16_FLOAT)
    assert V.VolumeTexture(Ctx, u16.view(np.float16)).format == V.FMT_R16_FLOAT
    assert V.VolumeTexture(Ctx, u16.astype(np.uint8)).format == V.FMT_R8_UNORM
    # fmt=FMT_R16_UNORM uploads the integers as they are
    vt = V.VolumeTexture(Ctx, u16, layout=V.LAYOUT_PACKED, fmt=V.FMT_R16_UNORM)
    assert vt.format == V.FMT_R16_UNORM == 3 and vt.dims == (4, 3, 2)
    assert fake.calls[-1] == (4, 3, 2, 3, V.LAYOUT_PACKED, u16.tobytes()[:4])
    # ... and takes nothing else
    for bad in (u16.astype(np.uint8), u16.view(np.float16), u16.astype(np.int16), u16.astype(np.float32), u16[0], u16[..., None].repeat(4, axis=3)):
        with pytest.raises(ValueError):
            V.VolumeTexture(Ctx, bad, fmt=V.FMT_R16_UNORM)
    with pytest.raises(ValueError):
        V.VolumeTexture(Ctx, u16, u16, fmt=V.FMT_R16_UNORM)
    # an explicit fmt that the array does not infer is refused; the one it infers is accepted
    with pytest.raises(ValueError):
        V.VolumeTexture(Ctx, u16, fmt=V.FMT_R8_UNORM)
    with pytest.raises(ValueError):
        V.VolumeTexture(Ctx, u16.astype(np.uint8), fmt=V.FMT_R16_FLOAT)
    assert V.VolumeTexture(Ctx, u16, fmt=V.FMT_R16_FLOAT).format == V.FMT_R16_FLOAT
    # from_raw: uint8 as before, uint16 as R16_UNORM, nothing else
    p = tmp_path / "v.raw"
    u16.tofile(p)
    assert V.VolumeTexture.from_raw(Ctx, str(p), dims=(4, 3, 2), dtype=np.uint16).format == V.FMT_R16_UNORM
    assert V.VolumeTexture.from_raw(Ctx, str(p), dims=(8, 3, 2)).format == V.FMT_R8_UNORM
    with pytest.raises(ValueError):
        V.VolumeTexture.from_raw(Ctx, str(p), dims=(4, 3, 3), dtype=np.uint16)
    with pytest.raises(ValueError):
        V.VolumeTexture.from_raw(Ctx, str(p), dims=(4, 3, 2), dtype=np.float16)
