"""The cell march's ray set-up with the short divisions (vokselis_amd/csrc/vk_exactdiv.hpp, vk_march_kernel_body.hpp) on the MI355X.

1. tests/exactdiv_device.hip, a stand-alone program: every helper against the plain `/` expression it replaces, on the device -- 0 differences.
2. Frames and per-pixel step counts with the knob `setup_generic` 0 and 1 bitwise equal, and within test_parity_gpu.py's bounds of the oracle:
   volumes 16^3, 8^3 and 24 x 17 x 9, images 96 x 64 and 70 x 50, four cameras (the bonsai camera; an eye on the z axis looking down it, aimed and snapped so
   that a pixel's direction has x and y components exactly 0 -- the guard must send its wave down the generic text; an eye inside the cube; an
   eye 1e4 away), PACKED_PAIRS and PACKED through vk_render and through vk_render_batch with 3 cameras at tile_size 32.
   (What the guard decides does not show in a frame for most out-of-range operands -- the unscaled chain goes wrong only near the ends of the
   exponent range -- so the range argument is the header's, and this holds the two texts to each other and to the oracle.)"""
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_helpers import TOL, V  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_helpers_equal_the_division_on_the_device(hip_built, tmp_path):
    exe = str(tmp_path / "exactdiv_device")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "vokselis_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "exactdiv_device.hip")], check=True, timeout=300)
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\w+): (\d+) cases, (\d+) differences$", r.stdout, re.M)}
    assert got["chain"] == ((1 << 23) * 11 * 3, 0), got          # every mantissa x exponents -40, -32 .. 40 x three helpers
    assert got["const"] == (8192 * 8193 // 2, 0), got            # every (x, W), W <= 8192
    assert got["dt"] == ((1 << 23) * 2 * 9 * 2, 0), got          # every mantissa x two binades x fn = 2^3 .. 2^11 x two forms


# ---- 2. the two texts of the set-up -------------------------------------------------------------------------------------------------

def _far_point(a, W, H, x, y):
    """q / q.w of pixel (x, y) and its offset from the eye: the kernel's arithmetic (generic text), redone here in binary32."""
    m = a[20:36]
    ndcx = f32(f32(f32(2) * f32(x + 0.5)) / f32(W)) - f32(1)
    ndcy = f32(1) - f32(f32(f32(2) * f32(y + 0.5)) / f32(H))
    q = [f32(f32(f32(f32(m[r] * ndcx) + f32(m[4 + r] * ndcy)) + m[8 + r]) + m[12 + r]) for r in range(4)]
    far = [f32(q[i] / q[3]) for i in range(3)]
    return far, [f32(far[i] - a[i]) for i in range(3)]


def _axis_camera(V, W, H):
    """An eye on the z axis through the cube's centre, at z = -1, aimed so that the ray of pixel (W // 2, H // 2) runs straight down the axis
    (an even image has no pixel in its middle: the camera is turned by half a pixel, solved for here), then moved by rounding noise onto that
    pixel's far point in x and y: the pixel's direction has x and y components exactly 0, its neighbours' are small."""
    import math

    x, y, zoom = W // 2, H // 2, 1.5

    def make(pitch, yaw):
        v = (math.sin(yaw) * math.cos(pitch), math.sin(pitch), math.cos(yaw) * math.cos(pitch))
        target = (0.5 + zoom * v[0], 0.5 + zoom * v[1], -1.0 + zoom * v[2])
        return np.frombuffer(V.Camera(zoom, pitch, yaw, target, W / H).get_proj_view_matrix(), np.float32).copy()

    def miss(pitch, yaw):
        d = _far_point(make(pitch, yaw), W, H, x, y)[1]
        return np.array([float(d[0]), float(d[1])]) / 100.0

    p = np.zeros(2)
    for _ in range(6):  # Newton on (pitch, yaw), the Jacobian by differences
        g, h = miss(*p), 1e-3
        J = np.stack([(miss(p[0] + h, p[1]) - g) / h, (miss(p[0], p[1] + h) - g) / h], axis=1)
        p = p - np.linalg.solve(J, g)
    a = make(*p)
    assert abs(a[0] - 0.5) < 1e-4 and abs(a[1] - 0.5) < 1e-4 and abs(a[2] + 1.0) < 1e-4, a[:3]
    far, d = _far_point(a, W, H, x, y)
    assert abs(d[0]) < 1e-3 and abs(d[1]) < 1e-3, d  # the pixel's ray is the axis, to rounding
    a[0], a[1] = far[0], far[1]
    d = _far_point(a, W, H, x, y)[1]
    assert d[0] == 0 and d[1] == 0 and d[2] > 50, d
    return a.tobytes()


def _cameras(V, W, H):
    aspect = W / H
    return {"bonsai": V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), aspect).get_proj_view_matrix(), "z axis": _axis_camera(V, W, H),
            "inside": V.Camera(0.3, 0.4, 2.5, (0.5, 0.5, 0.5), aspect).get_proj_view_matrix(),
            "far": V.Camera(1e4, 0.3, 0.7, (0.5, 0.5, 0.5), aspect).get_proj_view_matrix()}


def _volume(dims, seed):
    nx, ny, nz = dims
    return np.random.default_rng(seed).integers(0, 90, (nz, ny, nx)).astype(np.uint8)  # a third of the taps exactly transparent


def _bits(a):
    return a.view(np.uint32)


def _device_buffer(n_words, guard_words=4096):
    import torch

    t = torch.full((n_words + guard_words,), -1, dtype=torch.int32, device="cuda")  # 0xFF bytes: what nobody writes shows
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("W,H", [(96, 64), (70, 50)])
@pytest.mark.parametrize("dims", [(16, 16, 16), (8, 8, 8), (24, 17, 9)])
def test_short_and_generic_setup_agree(V, O, dims, W, H):
    vol = _volume(dims, seed=sum(dims))
    cams = _cameras(V, W, H)
    refs = {name: O.render(cam, vol, W, H, dt_scale=1.0) for name, cam in cams.items()}
    assert (refs["bonsai"][1] > 0).any() and (refs["z axis"][1] > 0).any() and (refs["inside"][1] > 0).all()
    flags = V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS
    for layout in (V.LAYOUT_PACKED_PAIRS, V.LAYOUT_PACKED):
        ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
        try:
            V.VolumeTexture(ctx, vol, layout=layout)
            frames = {}
            for generic in (0, 1):
                ctx.set_param("setup_generic", generic)
                for name, cam in cams.items():
                    ctx.set_camera_blob(cam)
                    V.RaycastPipeline(dt_scale=1.0, flags=flags | V.RENDER_COUNT).record(ctx)
                    img, steps = ctx.read_backbuffer().copy(), ctx.read_steps().copy()
                    V.RaycastPipeline(dt_scale=1.0, flags=flags).record(ctx)  # the production kernel
                    assert (_bits(ctx.read_backbuffer()) == _bits(img)).all(), (name, layout, generic)
                    frames[generic, name] = (img, steps)
                    ref, rsteps, _ = refs[name]
                    assert (steps == rsteps).all(), (name, layout, generic, int((steps != rsteps).sum()))
                    assert np.abs(img - ref).max() <= TOL, (name, layout, generic)
            for name in cams:
                assert (_bits(frames[0, name][0]) == _bits(frames[1, name][0])).all() and (frames[0, name][1] == frames[1, name][1]).all(), (name, layout)
            # ... and through a batch: three cameras, 32-pixel tiles, both texts, against the single frames
            pipe = V.RaycastPipeline(dt_scale=1.0, flags=flags)
            for names in (("bonsai", "z axis", "inside"), ("z axis", "inside", "far")):
                want = np.stack([_bits(frames[1, n][0]) for n in names])
                for generic in (0, 1):
                    ctx.set_param("setup_generic", generic)
                    buf = _device_buffer(3 * H * W * 4)
                    V.render_batch(ctx, pipe, [cams[n] for n in names], buf.data_ptr(), tile_size=32)
                    ctx.sync()
                    host = _host(buf)
                    assert (host[:want.size].reshape(want.shape) == want).all(), (names, layout, generic)
                    assert (host[want.size:] == 0xFFFFFFFF).all(), (names, layout, generic)
        finally:
            ctx.close()
