"""The mesh pass (vk_extract_isosurface) against a plain streaming read launched in the same run.  Volumes:
  standin    the 256^3 bonsai stand-in, u8 PACKED_PAIRS, iso 0.25
  ct         a 512 x 512 x 300 R16_UNORM volume (smooth shells plus noise), PACKED, iso 2500 / 65535
  ball       a 1024^3 u8 LINEAR volume, a ball field with a thin surface, iso 0.5
  tiny       a 64^3 u8 LINEAR ball: the floor of a call
Per volume:
  count_ms   the count-only call (triangles == NULL) between two events on the context's stream: count kernel, scan kernel, 16 bytes down
  fill_ms    the filling call into a caller's buffer of n triangles: count, scan, emit and the download of 36 n bytes
  wall_ms    the same two calls end to end on the host (allocation, launches, waits, free)
  bytes      the layout's array: the dense voxels (LINEAR) or the cell array (PACKED, PACKED_PAIRS; without its skip maps)
  stream_ms  the yardstick: a sum over an array of that many bytes with 16-byte loads (tools/ubench/stream_read.hip, built on first use
             and run as a child of this run), between two events
  ratio      count_ms / stream_ms and fill_ms / stream_ms
plus the triangle count and a checksum of the triangles.  What the code predicts is written in DESIGN.md section 21 before the run.
usage: tools/mesh_quick.py [--reps N] [--small]   (--small: 256^3 instead of 1024^3, for a quick look)"""
import ctypes as C
import json
import os
import subprocess
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: before the library)

import vokselis_amd as V
from vokselis_amd import _native as N

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
BIG = 256 if "--small" in sys.argv else 1024


def ct_volume():
    """tools/slice_quick.py's CT stand-in: shells around 1000 .. 4000 of 0 .. 65535 plus noise."""
    nx, ny, nz = 512, 512, 300
    z, y, x = np.linspace(-1, 1, nz, dtype=np.float32)[:, None, None], np.linspace(-1, 1, ny, dtype=np.float32)[None, :, None], np.linspace(-1, 1, nx, dtype=np.float32)[None, None, :]
    r = np.sqrt(x * x + y * y + 0.6 * z * z)
    v = 1000.0 + 1200.0 * (r < 0.8) + 1800.0 * ((r > 0.7) & (r < 0.8)) + 300.0 * np.sin(9.0 * x) * np.cos(7.0 * y)
    v = v + np.random.default_rng(5).integers(0, 60, v.shape).astype(np.float32)
    return np.clip(v, 0, 65535).astype(np.uint16)


def ball_volume(n):
    """1.3 - 1.6 r clipped to [0, 1] as u8, r the distance from the centre in half-extents, plane by plane."""
    out = np.empty((n, n, n), np.uint8)
    a = ((np.arange(n, dtype=np.float32) + 0.5) / n * 2.0 - 1.0) ** 2
    xy = a[:, None] + a[None, :]
    for k in range(n):
        out[k] = np.rint(np.clip(1.3 - 1.6 * np.sqrt(xy + a[k]), 0.0, 1.0) * 255.0).astype(np.uint8)
    return out


def cell_bytes(dims, cell):
    n = 64
    for d in dims:
        n *= ((d - 1) >> 2) + 2  # bricks of 4 cells per axis for low-corner voxels -1 .. d - 1
    return n * cell


def stream_ms(sizes):
    """{bytes: ms} from the streaming-read micro-benchmark."""
    here = os.path.dirname(os.path.abspath(__file__))
    src, exe = os.path.join(here, "ubench", "stream_read.hip"), os.path.join(here, "ubench", "_build", "stream_read")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    r = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=300)
    return {int(k): v for k, v in json.loads(r.stdout).items()}


def call(ctx, iso, buf):
    """One vk_extract_isosurface: count only (buf None), or filling buf.  Returns n."""
    req, n = N.VkMeshRequest(iso, 0), C.c_uint64(0)
    ptr = buf.ctypes.data_as(C.POINTER(C.c_float)) if buf is not None else None
    N.check(ctx.handle, N.lib().vk_extract_isosurface(ctx.handle, C.byref(req), None, ptr, len(buf) if buf is not None else 0, C.byref(n)))
    return int(n.value)


def gpu_ms(ctx, iso, buf, iters):
    best = 1e9
    for _ in range(3):
        ctx.timer_begin()
        for _ in range(iters):
            call(ctx, iso, buf)
        ctx.timer_end()
        best = min(best, ctx.timer_elapsed_ms() / iters)
    return best


def wall_ms(ctx, iso, buf, iters):
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(iters):
            call(ctx, iso, buf)
        best = min(best, (time.perf_counter() - t0) * 1e3 / iters)
    return best


def volumes():
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture.generate_standin(ctx, (256,) * 3, layout=V.LAYOUT_PACKED_PAIRS)
    yield "standin", ctx, cell_bytes((256,) * 3, 16), 255 ** 3, 0.25
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture(ctx, ct_volume(), layout=V.LAYOUT_PACKED, fmt=V.FMT_R16_UNORM)
    yield "ct", ctx, cell_bytes((512, 512, 300), 16), 511 * 511 * 299, 2500.0 / 65535.0
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture(ctx, ball_volume(BIG), layout=V.LAYOUT_LINEAR)
    yield "ball", ctx, BIG ** 3, (BIG - 1) ** 3, 0.5
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture(ctx, ball_volume(64), layout=V.LAYOUT_LINEAR)
    yield "tiny", ctx, 64 ** 3, 63 ** 3, 0.5


out = {"big": BIG}
names = []
for name, ctx, nbytes, cubes, iso in volumes():
    names.append(name)
    try:
        out[name + "_bytes"], out[name + "_cubes"] = nbytes, cubes
        n = call(ctx, iso, None)
        buf = np.zeros((max(n, 1), 3, 3), np.float32)
        assert call(ctx, iso, buf) == n
        out[name + "_triangles"] = n
        out[name + "_crc"] = "%08x" % zlib.crc32(buf[:n].tobytes())
        iters = 10 if n < 2000000 else 3
        for _ in range(3):
            call(ctx, iso, None)
            call(ctx, iso, buf)
        for rep in range(reps):
            out.setdefault(name + "_count_ms", []).append(round(gpu_ms(ctx, iso, None, 10), 4))
            out.setdefault(name + "_fill_ms", []).append(round(gpu_ms(ctx, iso, buf, iters), 4))
            out.setdefault(name + "_count_wall_ms", []).append(round(wall_ms(ctx, iso, None, 10), 4))
            out.setdefault(name + "_fill_wall_ms", []).append(round(wall_ms(ctx, iso, buf, iters), 4))
        for k in ("count", "fill", "count_wall", "fill_wall"):
            out[f"{name}_{k}_best_ms"] = min(out[f"{name}_{k}_ms"])
        del buf
    finally:
        ctx.close()
for rep in range(reps):  # the yardstick, once the contexts are closed: the same device, the same run
    ms = stream_ms([out[n + "_bytes"] for n in names])
    for n in names:
        out.setdefault(n + "_stream_ms", []).append(ms[out[n + "_bytes"]])
for n in names:
    out[n + "_stream_best_ms"] = min(out[n + "_stream_ms"])
    out[n + "_count_ratio"] = round(out[n + "_count_best_ms"] / out[n + "_stream_best_ms"], 3)
    out[n + "_fill_ratio"] = round(out[n + "_fill_best_ms"] / out[n + "_stream_best_ms"], 3)
print(json.dumps(out), flush=True)
