"""The histogram pass (vk_volume_histogram) against a plain streaming read launched in the same run.  Volumes:
  standin    the 256^3 bonsai stand-in, u8 PACKED_PAIRS
  ct         a 512 x 512 x 300 R16_UNORM volume (smooth shells plus noise), PACKED
  constant   a 1024^3 u8 LINEAR volume of one value
  random     a 1024^3 u8 LINEAR volume, uniform random
  tiny       a 64^3 u8 LINEAR volume, uniform random: the floor of a call
each at 256 and 4096 bins over [0, 1], whole volume.  Per volume and bin count:
  gpu_ms     the call between two events on the context's stream: the zero-fill of the result, the kernel, the download
  wall_ms    the blocking call end to end on the host (allocation, launch, wait, free)
and per volume
  bytes      the layout's array: the dense voxels (LINEAR) or the cell array (PACKED, PACKED_PAIRS; without its skip maps)
  stream_ms  the yardstick: a sum over an array of that many bytes with 16-byte loads (tools/ubench/stream_read.hip, built on first use
             and run as a child of this run), between two events
  ratio      gpu_ms / stream_ms at each bin count
plus the counts' checksum and whether the constant volume's time is within the random one's.  What the code predicts is written in
DESIGN.md section 20 before the run.
usage: tools/hist_quick.py [--reps N] [--small]   (--small: 256^3 instead of 1024^3, for a quick look)"""
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


def gpu_ms(ctx, bins, iters=10):
    best = 1e9
    for _ in range(3):
        ctx.timer_begin()
        for _ in range(iters):
            ctx.volume_histogram(bins, (0.0, 1.0))
        ctx.timer_end()
        best = min(best, ctx.timer_elapsed_ms() / iters)
    return best


def wall_ms(ctx, bins, iters=10):
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(iters):
            ctx.volume_histogram(bins, (0.0, 1.0))
        best = min(best, (time.perf_counter() - t0) * 1e3 / iters)
    return best


def volumes():
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture.generate_standin(ctx, (256,) * 3, layout=V.LAYOUT_PACKED_PAIRS)
    yield "standin", ctx, cell_bytes((256,) * 3, 16), 256 ** 3
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture(ctx, ct_volume(), layout=V.LAYOUT_PACKED, fmt=V.FMT_R16_UNORM)
    yield "ct", ctx, cell_bytes((512, 512, 300), 16), 512 * 512 * 300
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture(ctx, np.full((BIG,) * 3, 41, np.uint8), layout=V.LAYOUT_LINEAR)
    yield "constant", ctx, BIG ** 3, BIG ** 3
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture(ctx, np.random.default_rng(9).integers(0, 256, (BIG,) * 3, dtype=np.uint8), layout=V.LAYOUT_LINEAR)
    yield "random", ctx, BIG ** 3, BIG ** 3
    ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
    V.VolumeTexture(ctx, np.random.default_rng(10).integers(0, 256, (64,) * 3, dtype=np.uint8), layout=V.LAYOUT_LINEAR)
    yield "tiny", ctx, 64 ** 3, 64 ** 3


out = {"big": BIG}
for name, ctx, nbytes, voxels in volumes():
    try:
        out[name + "_bytes"] = nbytes
        for bins in (256, 4096):
            h = ctx.volume_histogram(bins, (0.0, 1.0))
            assert h.n_voxels == voxels == h.n_below + h.n_above + h.n_nan + int(h.counts.sum())
            out[f"{name}_{bins}_crc"] = "%08x" % zlib.crc32(h.counts.tobytes())
            for _ in range(5):
                ctx.volume_histogram(bins, (0.0, 1.0))
        for rep in range(reps):
            for bins in (256, 4096):
                out.setdefault(f"{name}_{bins}_gpu_ms", []).append(round(gpu_ms(ctx, bins), 4))
                out.setdefault(f"{name}_{bins}_wall_ms", []).append(round(wall_ms(ctx, bins), 4))
        for bins in (256, 4096):
            out[f"{name}_{bins}_gpu_best_ms"] = min(out[f"{name}_{bins}_gpu_ms"])
            out[f"{name}_{bins}_wall_best_ms"] = min(out[f"{name}_{bins}_wall_ms"])
    finally:
        ctx.close()
names = ("standin", "ct", "constant", "random", "tiny")
for rep in range(reps):  # the yardstick, once the contexts are closed: the same device, the same run
    ms = stream_ms([out[n + "_bytes"] for n in names])
    for n in names:
        out.setdefault(n + "_stream_ms", []).append(ms[out[n + "_bytes"]])
for n in names:
    out[n + "_stream_best_ms"] = min(out[n + "_stream_ms"])
    for bins in (256, 4096):
        out[f"{n}_{bins}_ratio"] = round(out[f"{n}_{bins}_gpu_best_ms"] / out[n + "_stream_best_ms"], 3)
for bins in (256, 4096):
    out[f"constant_within_random_{bins}"] = bool(out[f"constant_{bins}_gpu_best_ms"] <= out[f"random_{bins}_gpu_best_ms"])
print(json.dumps(out), flush=True)
