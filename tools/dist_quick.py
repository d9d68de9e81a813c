"""The distance pass (vk_distance_transform), kernel by kernel, beside its yardsticks.  Volumes, u8, LINEAR and PACKED
each:
  standin      the 256^3 bonsai stand-in at the threshold 0.3
  perc512      a 512^3 site-percolation field at density 79 / 256 = 0.309
  perc1024     the same at 1024^3
Per volume and layout, for VK_DIST_OUTSIDE at spacing 1 1 1:
  <phase>_ms   each phase alone -- column (along z), line_y, line_x (transpose, lines, transpose back), stats -- between the context's
               timer events (vk_debug_set_param "dist_timing" k), best of --reps calls; the calls ask for the result only; line_x_plain_ms:
               the x pass without its transposes ("dist_x_plain" 1), the line function along rows
  call_ms      the blocking call end to end on the host, result only
  close_ms     VK_DIST_CLOSE at radius 2 as a whole call (two rounds and the mask kernel), counts only, and its mask kernel alone (mask_ms)
  n_fg, max_d2 the result
and per volume and layout
  stream_ms    a sum over the layout's array with 16-byte loads (tools/ubench/stream_read.hip, as tools/filter_quick.py runs it), and
  stream_d2_ms the same over an array of the distance array's size, 4 bytes a voxel: the line passes read one and write two of those
  cpu_ms       scipy.ndimage.distance_transform_edt on one CPU thread on the same set -- not for 1024^3 -- whose rounded square must be
               the library's d2_out (cpu_agrees)
usage: tools/dist_quick.py [--reps N] [--small]   (--small: no 1024^3)"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: before the library)

import vokselis_amd as V

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
PHASES = ((1, "column"), (2, "line_y"), (3, "line_x"), (7, "stats"))


def cell_bytes(dims, cell):
    n = 64
    for d in dims:
        n *= ((d - 1) >> 2) + 2
    return n * cell


def stream_ms(sizes):
    src, exe = os.path.join(HERE, "ubench", "stream_read.hip"), os.path.join(HERE, "ubench", "_build", "stream_read")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    r = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=300)
    return {int(k): v for k, v in json.loads(r.stdout).items()}


def percolation(n):
    rng = np.random.default_rng(31)
    vol = np.empty((n, n, n), np.uint8)
    for z in range(n):  # a plane at a time: no float64 copy of the whole field
        vol[z] = np.where(rng.integers(0, 256, (n, n), dtype=np.uint8) < 79, 255, 0)
    return vol


def volumes():
    from oracle import oracle as O

    yield "standin", O.volume_standin_u8(256), 0.3
    yield "perc512", percolation(512), 0.5
    if "--small" not in sys.argv:
        yield "perc1024", percolation(1024), 0.5


out = {}
names = []
for vname, vol, lo in volumes():
    dims = tuple(reversed(vol.shape))
    d2 = None
    for layout, lname in ((V.LAYOUT_LINEAR, "linear"), (V.LAYOUT_PACKED, "packed")):
        name = f"{vname}_{lname}"
        names.append(name)
        print(name, file=sys.stderr, flush=True)
        out[name + "_bytes"] = vol.size if layout == V.LAYOUT_LINEAR else cell_bytes(dims, 8)
        out[name + "_d2_bytes"] = vol.size * 4
        ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
        try:
            V.VolumeTexture(ctx, vol, layout=layout)
            req = V.distance_request(lo)
            res = V.native.VkDistanceResult()
            call = lambda r=req, d=None: V.native.check(ctx.handle, V.native.lib().vk_distance_transform(ctx.handle, C.byref(r), None, d, None, C.byref(res)))
            call()
            out[name + "_n_fg"], out[name + "_max_d2"] = int(res.n_foreground), int(res.max_d2)
            for k, phase in PHASES:
                ctx.set_param("dist_timing", k)
                best = 1e9
                for _ in range(reps):
                    call()
                    best = min(best, ctx.timer_elapsed_ms())
                out[f"{name}_{phase}_ms"] = round(best, 4)
            ctx.set_param("dist_x_plain", 1)
            ctx.set_param("dist_timing", 3)
            best = 1e9
            for _ in range(reps):
                call()
                best = min(best, ctx.timer_elapsed_ms())
            out[name + "_line_x_plain_ms"] = round(best, 4)
            ctx.set_param("dist_x_plain", 0)
            ctx.set_param("dist_timing", 0)
            out[name + "_kernels_ms"] = round(sum(out[f"{name}_{p}_ms"] for _, p in PHASES), 4)
            best = 1e9
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                best = min(best, (time.perf_counter() - t0) * 1e3)
            out[name + "_call_ms"] = round(best, 3)
            close = V.distance_request(lo, op="close", radius=2.0)
            best = 1e9
            for _ in range(reps):
                t0 = time.perf_counter()
                call(close)
                best = min(best, (time.perf_counter() - t0) * 1e3)
            out[name + "_close_ms"] = round(best, 3)
            out[name + "_close_added"] = int(res.n_added)
            ctx.set_param("dist_timing", 7)
            call(close)
            out[name + "_mask_ms"] = round(ctx.timer_elapsed_ms(), 4)
            ctx.set_param("dist_timing", 0)
            if layout == V.LAYOUT_LINEAR and vol.size <= 512 ** 3:
                d2 = np.zeros(vol.shape, np.uint32)
                call(req, d2.ctypes.data)
        finally:
            ctx.close()
    if d2 is not None:
        try:
            from scipy import ndimage

            fg = vol.astype(np.float32) >= np.float32(lo) * np.float32(255.0)
            t0 = time.perf_counter()
            edt = ndimage.distance_transform_edt(~fg)
            out[vname + "_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            out[vname + "_cpu_agrees"] = bool((np.rint(edt ** 2).astype(np.uint32) == d2).all())
        except ImportError:
            out[vname + "_cpu_ms"] = None
    del vol, d2
sizes = sorted({out[n + "_bytes"] for n in names} | {out[n + "_d2_bytes"] for n in names})
for rep in range(reps):
    ms = stream_ms(sizes)
    for n in names:
        out[n + "_stream_ms"] = min(out.get(n + "_stream_ms", 1e9), ms[out[n + "_bytes"]])
        out[n + "_stream_d2_ms"] = min(out.get(n + "_stream_d2_ms", 1e9), ms[out[n + "_d2_bytes"]])
print(json.dumps(out), flush=True)
