"""The volume filter pass (vk_volume_filter) against a plain streaming read launched in the same run.  Volumes:
  standin    the 256^3 bonsai stand-in, u8, LINEAR and PACKED
  fog        a 1024^3 u8 fog, LINEAR and PACKED
Filters: Gaussians of radius 1, 2, 4 and 6 on all three axes (the three tile classes of vk_filter.hpp), and MEDIAN3.  Per volume, layout
and filter:
  kernel_ms  the kernel alone, between two events the call records around its launch (vk_debug_set_param "filter_timing"); the call
             itself goes to dense_out without VK_FILTER_INSTALL, so nothing but the kernel lies between the events
  ratio      kernel_ms / stream_ms
and per volume and layout
  bytes      the layout's array: the dense voxels (LINEAR) or the cell array (PACKED; without its skip maps)
  stream_ms  the yardstick: a sum over an array of that many bytes with 16-byte loads (tools/ubench/stream_read.hip, built on first use
             and run as a child of this run), between two events; dense_stream_ms the same over the dense bytes (what the kernel writes)
  install_ms the blocking VK_FILTER_INSTALL call of the radius-1 Gaussian end to end on the host: allocation, kernel, re-layout, census
             and skip maps, the old volume freed
  upload_ms  vk_volume_upload of the same dense array end to end: what the caller's host round trip costs without the copy down
plus whether all radii 0 returns the stored volume and a checksum of every output.  What the code predicts is written in DESIGN.md
section 22 before the run.
usage: tools/filter_quick.py [--reps N] [--small]   (--small: 256^3 instead of 1024^3, for a quick look)"""
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
FILTERS = [("r1", 1, 0.5), ("r2", 2, 0.8), ("r4", 4, 1.5), ("r6", 6, 2.0), ("median3", 0, 0.0)]


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


def run_filter(ctx, radius, sigma):
    if radius == 0:
        return ctx.median_volume(install=False, out=True)
    w = V.gaussian_weights(sigma, radius)
    return ctx.filter_volume((w, w, w), install=False, out=True)


def volumes():
    for layout, lname in ((V.LAYOUT_LINEAR, "linear"), (V.LAYOUT_PACKED, "packed")):
        ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
        V.VolumeTexture.generate_standin(ctx, (256,) * 3, layout=layout)
        yield "standin_" + lname, ctx, (256,) * 3, layout
        ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
        V.VolumeTexture.generate_fog(ctx, (BIG,) * 3, layout=layout)
        yield "fog_" + lname, ctx, (BIG,) * 3, layout


out = {"big": BIG}
names = []
for name, ctx, dims, layout in volumes():
    try:
        names.append(name)
        dense = dims[0] * dims[1] * dims[2]
        out[name + "_bytes"] = dense if layout == V.LAYOUT_LINEAR else cell_bytes(dims, 8)
        out[name + "_dense_bytes"] = dense
        stored = ctx.filter_volume((None, None, None), install=False, out=True)  # all radii 0: the stored volume
        ctx.set_param("filter_timing", 1)
        for fname, radius, sigma in FILTERS:
            got = run_filter(ctx, radius, sigma)
            out[f"{name}_{fname}_crc"] = "%08x" % zlib.crc32(got.tobytes())
            del got
        for rep in range(reps):
            for fname, radius, sigma in FILTERS:
                best = 1e9
                for _ in range(2):
                    run_filter(ctx, radius, sigma)
                    best = min(best, ctx.timer_elapsed_ms())
                out.setdefault(f"{name}_{fname}_kernel_ms", []).append(round(best, 4))
        for fname, _, _ in FILTERS:
            out[f"{name}_{fname}_kernel_best_ms"] = min(out[f"{name}_{fname}_kernel_ms"])
        ctx.set_param("filter_timing", 0)
        # the install, end to end, against an upload of the same dense array
        w = V.gaussian_weights(0.5, 1)
        for rep in range(reps):
            t0 = time.perf_counter()
            ctx.filter_volume((w, w, w), install=True)
            ctx.sync()
            out.setdefault(name + "_install_ms", []).append(round((time.perf_counter() - t0) * 1e3, 3))
        for rep in range(reps):
            t0 = time.perf_counter()
            V.VolumeTexture(ctx, stored, layout=layout)
            ctx.sync()
            out.setdefault(name + "_upload_ms", []).append(round((time.perf_counter() - t0) * 1e3, 3))
        again = ctx.filter_volume((None, None, None), install=False, out=True)
        out[name + "_identity_ok"] = bool((again == stored).all())
        out[name + "_install_best_ms"] = min(out[name + "_install_ms"])
        out[name + "_upload_best_ms"] = min(out[name + "_upload_ms"])
        del stored, again
    finally:
        ctx.close()
sizes = sorted({out[n + "_bytes"] for n in names} | {out[n + "_dense_bytes"] for n in names})
for rep in range(reps):  # the yardstick, once the contexts are closed: the same device, the same run
    ms = stream_ms(sizes)
    for n in names:
        out.setdefault(n + "_stream_ms", []).append(ms[out[n + "_bytes"]])
        out.setdefault(n + "_dense_stream_ms", []).append(ms[out[n + "_dense_bytes"]])
for n in names:
    out[n + "_stream_best_ms"] = min(out[n + "_stream_ms"])
    out[n + "_dense_stream_best_ms"] = min(out[n + "_dense_stream_ms"])
    for fname, _, _ in FILTERS:
        out[f"{n}_{fname}_ratio"] = round(out[f"{n}_{fname}_kernel_best_ms"] / out[n + "_stream_best_ms"], 3)
        out[f"{n}_{fname}_dense_ratio"] = round(out[f"{n}_{fname}_kernel_best_ms"] / out[n + "_dense_stream_best_ms"], 3)
print(json.dumps(out), flush=True)
