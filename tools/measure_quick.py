"""The measuring pass (vk_measure_components), phase by phase, beside three yardsticks.  Volumes, LINEAR and PACKED each,
as u8 and as f16 (the same values v / 255 rounded to f16):
  standin      the 256^3 bonsai stand-in at the threshold 0.3
  spheres512   a 512^3 field of packed spheres: centres on a jittered grid of pitch 24, radii 10 .. 14 (tools/split_quick.py's)
  spheres1024  the same at 1024^3
Per volume, format and layout, at connectivity 6, the library labelling the range itself:
  <phase>_ms   each phase alone between the context's timer events (vk_debug_set_param "measure_timing" k) -- tile (tile and seam), flatten
               (flatten and scan), number (number and stats), init, measure -- best of --reps calls with room for every record
  call_ms      the blocking call end to end on the host, records included
  totals       regions, foreground voxels
  stats_ms     vk_label_components' stats kernel alone on the same data ("label_timing" 6): the kernel whose raster order, run detection
               and table scheme the measure kernel takes over
  bound_ms     the measure kernel's streaming bound: 4 bytes of label and the texel per voxel, and for a foreground voxel the four
               neighbour rows (+-y, +-z: 16 bytes), over stream_ms's rate
  stream_ms    a sum over an array of the label array's size (4 bytes per voxel) with 16-byte loads (tools/ubench/stream_read.hip)
and for the 256^3 stand-in
  cpu_ms       the C restatement (tests/measure_restatement.c, gcc -O2, one thread) over labels that the library produced, with its
               records, which must be the library's
usage: tools/measure_quick.py [--reps N] [--small] [--only NAME]   (--small: no 1024^3; --only: one of the three volumes)"""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: before the library)

import vokselis_amd as V

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
PHASES = ("tile", "flatten", "number", "init", "measure")


def stream_ms(sizes):
    src, exe = os.path.join(HERE, "ubench", "stream_read.hip"), os.path.join(HERE, "ubench", "_build", "stream_read")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    r = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=300)
    return {int(k): v for k, v in json.loads(r.stdout).items()}


def spheres(n, pitch=24):
    """tools/split_quick.py's field, seed and all."""
    rng = np.random.default_rng(27)
    vol = np.zeros((n, n, n), np.uint8)
    cells = (n + pitch - 1) // pitch
    for cz in range(cells):
        for cy in range(cells):
            for cx in range(cells):
                c = np.array([cz, cy, cx]) * pitch + pitch // 2 + rng.integers(-3, 4, 3)
                r = int(rng.integers(10, 15))
                lo, hi = np.maximum(c - r, 0), np.minimum(c + r + 1, n)
                if (hi <= lo).any():
                    continue
                z, y, x = np.ogrid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
                ball = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r
                vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]][ball] = 255
    return vol


def volumes():
    from oracle import oracle as O

    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
    if only in (None, "standin"):
        yield "standin", O.volume_standin_u8(256), 0.3
    if only in (None, "spheres512"):
        yield "spheres512", spheres(512), 0.5
    if only in (None, "spheres1024") and "--small" not in sys.argv:
        yield "spheres1024", spheres(1024), 0.5


out = {}
names = []
for vname, vol8, lo in volumes():
    for fmt in ("u8", "f16"):
        vol = vol8 if fmt == "u8" else (vol8.astype(np.float32) / 255.0).astype(np.float16)
        texel = 1 if fmt == "u8" else 2
        for layout, lname in ((V.LAYOUT_LINEAR, "linear"), (V.LAYOUT_PACKED, "packed")):
            name = f"{vname}_{fmt}_{lname}"
            names.append(name)
            print(name, file=sys.stderr, flush=True)
            out[name + "_bytes"] = vol.size * 4
            ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
            try:
                V.VolumeTexture(ctx, vol, layout=layout)
                req, res = V.measure_request(lo, math.inf), V.VkMeasureResult()
                V.native.check(ctx.handle, V.native.lib().vk_measure_components(ctx.handle, C.byref(req), None, None, None, 0, C.byref(res)))
                room = max(int(res.n_regions), 1)
                table = (V.VkRegion * room)()
                call = lambda: V.native.check(ctx.handle, V.native.lib().vk_measure_components(ctx.handle, C.byref(req), None, None, table, room, C.byref(res)))
                call()
                out[name + "_totals"] = [int(res.n_regions), int(res.n_foreground)]
                for k, phase in enumerate(PHASES, 1):
                    ctx.set_param("measure_timing", k)
                    best = 1e9
                    for _ in range(reps):
                        call()
                        best = min(best, ctx.timer_elapsed_ms())
                    out[f"{name}_{phase}_ms"] = round(best, 4)
                ctx.set_param("measure_timing", 0)
                best = 1e9
                for _ in range(reps):
                    t0 = time.perf_counter()
                    call()
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                out[name + "_call_ms"] = round(best, 3)
                lreq, lres = V.native.VkLabelRequest(), V.VkLabelResult()
                lreq.lo, lreq.hi, lreq.connectivity = lo, math.inf, 6
                ctx.set_param("label_timing", 6)
                best = 1e9
                for _ in range(reps):
                    V.native.check(ctx.handle, V.native.lib().vk_label_components(ctx.handle, C.byref(lreq), None, None, None, 0, None, C.byref(lres)))
                    best = min(best, ctx.timer_elapsed_ms())
                ctx.set_param("label_timing", 0)
                out[name + "_stats_ms"] = round(best, 4)
                out[name + "_bound_bytes"] = vol.size * (4 + texel) + int(res.n_foreground) * 16
                if vname == "standin" and lname == "linear":
                    import measure_helpers as MH

                    labels = ctx.label_components(lo, labels=True).labels
                    os.makedirs(os.path.join(HERE, "ubench", "_build"), exist_ok=True)
                    L = MH.build_restatement(os.path.join(HERE, "ubench", "_build"))
                    t0 = time.perf_counter()
                    ref, fg = MH.restate(L, vol, fmt, labels, int(res.n_regions))
                    out[name + "_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    out[name + "_cpu_records_agree"] = bool((MH.table_array(table, int(res.records_written)) == ref).all()) and fg == int(res.n_foreground)
            finally:
                ctx.close()
    del vol8
sizes = sorted({out[n + "_bytes"] for n in names})
for rep in range(reps):
    ms = stream_ms(sizes)
    for n in names:
        out[n + "_stream_ms"] = min(out.get(n + "_stream_ms", 1e9), ms[out[n + "_bytes"]])
for n in names:
    out[n + "_bound_ms"] = round(out[n + "_stream_ms"] * out[n + "_bound_bytes"] / out[n + "_bytes"], 4)
print(json.dumps(out), flush=True)
