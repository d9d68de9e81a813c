"""The clip box (vk_set_clip_box) without a GPU: vk_tiles_active_clip through the built library, the host geometry
under a box under AddressSanitizer and UndefinedBehaviorSanitizer (tests/clip_hostmath_fuzz.cpp), the setter's validation as far as it
runs without a device, and the numpy references under a box (tests/np_clip_reference.py) over the shared cases (tests/clip_cases.py):
the unit box reproduces the unclipped frames and steps exactly, and no clipped case is an empty picture."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clip_cases as CC
import np_clip_reference as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 176, 104


def _active(lib, blob, ts, box="plain"):
    tx, ty = -(-W // ts), -(-H // ts)
    act, n = (C.c_ubyte * (tx * ty))(), C.c_uint32()
    if box == "plain":
        rc = lib.vk_tiles_active(blob, 0, W, H, ts, act, C.byref(n))
    else:
        from vokselis_amd import _native as N

        rc = lib.vk_tiles_active_clip(blob, 0, W, H, ts, None if box is None else C.byref(N.clip_box(*box)), act, C.byref(n))
    assert rc == 0
    act = np.frombuffer(act, np.uint8).reshape(ty, tx).astype(bool)
    assert n.value == act.sum()
    return act


def _random_box(rng, kind):
    lo, hi = np.sort(rng.uniform(0.0, 1.0, (2, 3)), axis=0).astype(np.float32)
    if kind == 1:  # a slab
        a = int(rng.integers(0, 3))
        lo[a] = rng.uniform(0.3, 0.7)
        hi[a] = lo[a] + rng.uniform(1e-4, 0.02)
    if kind == 2:  # on 1/8 boundaries
        lo = (rng.integers(0, 7, 3) / 8.0).astype(np.float32)
        hi = np.minimum(lo + rng.integers(1, 8, 3) / 8.0, 1.0).astype(np.float32)
    hi = np.where(hi > lo, hi, np.nextafter(lo, np.float32(2.0))).astype(np.float32)
    return tuple(float(v) for v in lo), tuple(float(v) for v in np.minimum(hi, np.float32(1.0)))


def test_tiles_active_clip_null_and_unit_box_are_tiles_active(hip_built, O):
    rng = np.random.default_rng(0xC11B)
    for case in range(40):
        blob = O.camera_blob(float(rng.choice([0.2, 0.45, 1.0, 3.0])), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(0, 6.283)),
                             tuple(float(v) for v in rng.uniform(0.0, 1.0, 3)), W / H)
        for ts in (8, 32):
            plain = _active(hip_built, blob, ts)
            assert (_active(hip_built, blob, ts, None) == plain).all() and (_active(hip_built, blob, ts, NC.UNIT) == plain).all()


def test_tiles_active_clip_covers_every_ray_that_hits_the_box(hip_built, O):
    """No pixel whose float64 ray hits the box lies in an inactive tile, and a box never activates a tile: seeded cameras around the cube,
    inside the cube, inside the box, edge-on, and with box corners behind the eye."""
    rng = np.random.default_rng(0xC11C)
    seen = dict(eye_in_box=0, eye_in_cube=0, edge_on=0, corner_behind=0, fewer=0)
    for case in range(200):
        box = _random_box(rng, case % 4)
        lo, hi = np.array(box[0], np.float64), np.array(box[1], np.float64)
        mid = tuple(float(v) for v in (lo + hi) / 2)
        kind = case % 5
        zoom, pitch, yaw, tgt = float(rng.uniform(0.3, 3.0)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(0, 6.283)), (0.5, 0.5, 0.5)
        if kind == 1:    # eye inside the cube
            zoom, tgt = float(rng.uniform(0.05, 0.4)), tuple(float(v) for v in rng.uniform(0.2, 0.8, 3))
        elif kind == 2:  # eye inside the box
            zoom, tgt = 0.4 * float((hi - lo).min()), mid
        elif kind == 3:  # edge-on: axis-aligned, the eye level with the box's centre
            pitch, yaw, tgt = 0.0, float(rng.integers(0, 4)) * 1.5707963, mid
            seen["edge_on"] += 1
        elif kind == 4:  # close to the box: corners behind the eye
            zoom, tgt = float(rng.uniform(0.2, 0.6)), tuple(float(v) for v in np.array(mid) + rng.uniform(-0.3, 0.3, 3))
        blob = O.camera_blob(zoom, pitch, yaw, tgt, W / H)
        cam = np.frombuffer(blob, np.float32).astype(np.float64)
        eye, pv = cam[:3], cam[4:20].reshape(4, 4)
        in_box = bool(((eye > lo) & (eye < hi)).all())
        seen["eye_in_box"] += in_box
        seen["eye_in_cube"] += bool(((eye > 0) & (eye < 1)).all()) and not in_box
        corners = np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2], 1.0] for c in range(8)])
        seen["corner_behind"] += bool(((corners @ pv)[:, 3] <= 0).any()) and not in_box
        hit = NC.ray_hits_f64(blob, W, H, box)
        for ts in (8, 32):
            tx, ty = -(-W // ts), -(-H // ts)
            act, plain = _active(hip_built, blob, ts, box), _active(hip_built, blob, ts)
            touched = np.zeros((ty, tx), bool)
            for j in range(ty):
                for i in range(tx):
                    touched[j, i] = hit[j * ts:(j + 1) * ts, i * ts:(i + 1) * ts].any()
            assert not (touched & ~act).any(), (case, ts, box, zoom, pitch, yaw, tgt)
            assert not (act & ~plain).any() and act.sum() <= plain.sum(), (case, ts, box)
            seen["fewer"] += int(act.sum() < plain.sum())
    assert min(seen["eye_in_box"], seen["eye_in_cube"], seen["corner_behind"]) >= 10 and seen["edge_on"] == 40 and seen["fewer"] >= 100, seen
    # the compute twin marches [-1, 1]^3 under another ray generator: every tile stays active under any box; bad boxes and arguments are refused
    from vokselis_amd import _native as N

    act = (C.c_ubyte * 9)()
    blob = O.camera_blob(3.0, -0.5, 1.0, (0.0, 0.0, 0.0), 1.0)
    assert hip_built.vk_tiles_active_clip(blob, 1, 24, 24, 8, C.byref(N.clip_box(*CC.ROI)), act, None) == 0 and all(act)
    assert hip_built.vk_tiles_active_clip(None, 0, 24, 24, 8, None, act, None) != 0 and hip_built.vk_tiles_active_clip(blob, 0, 24, 24, 12, None, act, None) != 0
    for lo, hi in (((0.5, 0.0, 0.0), (0.5, 1.0, 1.0)), ((0.6, 0.0, 0.0), (0.5, 1.0, 1.0)), ((-0.1, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.5, 1.0)),
                   ((0.0, float("nan"), 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, float("inf")))):
        b = N.VkClipBox()
        b.lo[:], b.hi[:] = lo, hi
        assert hip_built.vk_tiles_active_clip(blob, 0, 24, 24, 8, C.byref(b), act, None) == -1, (lo, hi)


@pytest.fixture(scope="module")
def fuzz_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("clip_hostmath") / "clip_hostmath_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "clip_hostmath_fuzz.cpp")], check=True)
    return exe


@pytest.mark.parametrize("seed", ["88172645463325252", "0x9E3779B97F4A7C15", "20261019"])
def test_clip_hostmath_under_sanitizers(fuzz_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz_exe, "400", seed], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith("OK (400 cases)") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_clip_box_validation_without_a_device(hip_built):
    """What Context.set_clip_box checks before the library sees the box (vokselis_amd._native.clip_box), and the C entry points on a NULL
    context: an error code, never a crash."""
    from vokselis_amd import _native as N

    assert C.sizeof(N.VkClipBox) == 24
    b = N.clip_box((0.25, 0.3, 0.1), (0.8, 0.75, 0.6))
    assert tuple(b.lo) == tuple(np.float32(v) for v in (0.25, 0.3, 0.1)) and tuple(b.hi) == tuple(np.float32(v) for v in (0.8, 0.75, 0.6))
    assert tuple(N.clip_box(*NC.UNIT).hi) == (1.0, 1.0, 1.0)
    for lo, hi in (((0.5, 0.0, 0.0), (0.5, 1.0, 1.0)),                      # lo == hi
                   ((0.6, 0.0, 0.0), (0.5, 1.0, 1.0)),                      # lo > hi
                   ((-0.1, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0001)),
                   ((0.0, float("nan"), 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (float("inf"), 1.0, 1.0)),
                   ((0.0, 0.0), (1.0, 1.0, 1.0)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)),
                   ((0.5, 0.0, 0.0), (0.5 + 1e-9, 1.0, 1.0))):                # distinct doubles, one f32: empty as the library compares it
        with pytest.raises(ValueError):
            N.clip_box(lo, hi)
    assert hip_built.vk_set_clip_box(None, None) == -1 and hip_built.vk_set_clip_box(None, C.byref(b)) == -1
    assert hip_built.vk_get_clip_box(None, None, None) == -1


def test_references_under_the_unit_box_are_the_unclipped_ones(O):
    """The per-axis intersection with lo = 0, hi = 1 is the scalar one, operation for operation: frames and steps are equal exactly; and
    the substitution is undone after every call."""
    from oracle import np_restatement as R

    original = R.intersect_box
    n = 0
    for c in CC.CASES:
        if c.box != "unit" and not c.half:
            continue
        n += 1
        rgb, steps = CC.reference(O, c, box=NC.UNIT)
        rgb0, steps0 = CC.reference(O, c, box=None)
        assert (steps == steps0).all() and (rgb.view(np.uint64) == rgb0.view(np.uint64)).all(), c
        assert R.intersect_box is original
    assert n >= 5
    with pytest.raises(ZeroDivisionError):
        with NC.clip_box(CC.ROI):
            assert R.intersect_box is not original
            1 / 0
    assert R.intersect_box is original


def test_no_clipped_case_is_an_empty_picture(O):
    """The condition on the inputs of tests/test_clip_gpu.py: in every case not tagged as a deliberate miss at least 2 % of the tile's
    pixels take a step, and under every box but the unit cube at least 2 % of them differ from the unclipped reference."""
    families, boxes, cameras, volumes, dts = set(), set(), set(), set(), set()
    for c in CC.CASES:
        rgb, steps = CC.reference(O, c)
        rgb0, steps0 = CC.reference(O, c, box=None)
        m = CC.tile_mask(c)
        assert (steps[~m] == 0).all() and (rgb[~m] == 0).all()
        hits = float((steps[m] > 0).mean())
        differ = float(((rgb[m] != rgb0[m]).any(axis=-1) | (steps[m] != steps0[m])).mean())
        if not c.miss:
            assert hits >= 0.02, (c, hits)
            if c.box != "unit":
                assert differ >= 0.02, (c, differ)
        families.add(c.family); boxes.add(c.box); cameras.add(c.camera); volumes.add(c.volume); dts.add(c.dt)
    assert families == set(CC.FAMILIES) and boxes == set(CC.BOXES) and cameras == set(CC.CAMERAS) and volumes == set(CC.volumes(O)) and dts == {0.15, 0.5, 1.7}
    assert sum(c.tile is not None for c in CC.CASES) >= 1 and {c.family for c in CC.CASES if c.half} >= {"table", "lit", "mip", "iso"}
