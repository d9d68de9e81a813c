"""The split pass (vk_split_components), phase by phase, beside three yardsticks.  Volumes, u8, LINEAR and PACKED each:
  standin      the 256^3 bonsai stand-in at the threshold 0.3
  spheres512   a 512^3 field of packed spheres: centres on a jittered grid of pitch 24, radii 10 .. 14, so that neighbours touch
  spheres1024  the same at 1024^3
Per volume, layout and radius (3, 8), at connectivity 6:
  <phase>_ms   each phase alone between the context's timer events (vk_debug_set_param "split_timing" k) -- distance, markers, growth (every
               round, with the host's looks at the counts), residue, merge, number (number and stats), cut -- best of --reps calls that ask
               for the totals only
  rounds, launches, round_ms   the rounds of the rule, the growth launches (whole batches of 8) and growth_ms per launch
  call_ms      the blocking call end to end on the host, totals only
  totals       regions, markers, residue regions, cut voxels
and per volume and layout
  before_ms    vk_distance_transform(INSIDE) + vk_label_components, blocking, totals only, in the same run: what the call costs before any growth
  stream_ms    a sum over an array of the state array's size (4 bytes per voxel) with 16-byte loads (tools/ubench/stream_read.hip)
  cpu_ms       the C restatement (tests/split_restatement.c, gcc -O2, one thread) at radius 3 -- the stand-in only: its distance pass is
               quadratic in a line's length -- with its totals, which must be the library's
usage: tools/split_quick.py [--reps N] [--small]   (--small: no 1024^3)"""
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
PHASES = ("distance", "markers", "growth", "residue", "merge", "number", "cut")
BATCH = 8


def stream_ms(sizes):
    src, exe = os.path.join(HERE, "ubench", "stream_read.hip"), os.path.join(HERE, "ubench", "_build", "stream_read")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    r = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=300)
    return {int(k): v for k, v in json.loads(r.stdout).items()}


def spheres(n, pitch=24):
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

    yield "standin", O.volume_standin_u8(256), 0.3
    yield "spheres512", spheres(512), 0.5
    if "--small" not in sys.argv:
        yield "spheres1024", spheres(1024), 0.5


out = {}
names = []
for vname, vol, lo in volumes():
    for layout, lname in ((V.LAYOUT_LINEAR, "linear"), (V.LAYOUT_PACKED, "packed")):
        name = f"{vname}_{lname}"
        names.append(name)
        print(name, file=sys.stderr, flush=True)
        out[name + "_bytes"] = vol.size * 4
        ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
        try:
            V.VolumeTexture(ctx, vol, layout=layout)
            for radius in (3.0, 8.0):
                key = f"{name}_r{radius:g}"
                req = V.split_request(lo, math.inf, radius=radius)
                res = V.VkSplitResult()
                call = lambda: V.native.check(ctx.handle, V.native.lib().vk_split_components(ctx.handle, C.byref(req), None, None, None, 0, None, C.byref(res)))
                call()
                out[key + "_totals"] = [int(res.n_regions), int(res.n_markers), int(res.n_residue_regions), int(res.n_cut)]
                out[key + "_rounds"] = int(res.rounds)
                out[key + "_launches"] = BATCH * (int(res.rounds) // BATCH + 1)
                for k, phase in enumerate(PHASES, 1):
                    ctx.set_param("split_timing", k)
                    best = 1e9
                    for _ in range(reps):
                        call()
                        best = min(best, ctx.timer_elapsed_ms())
                    out[f"{key}_{phase}_ms"] = round(best, 4)
                ctx.set_param("split_timing", 0)
                out[key + "_round_ms"] = round(out[key + "_growth_ms"] / out[key + "_launches"], 4)
                best = 1e9
                for _ in range(reps):
                    t0 = time.perf_counter()
                    call()
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                out[key + "_call_ms"] = round(best, 3)
            # what the call costs before any growth: the inside distance and the labelling, totals only
            dreq, dres = V.distance_request(lo, math.inf, op="inside"), V.VkDistanceResult()
            lreq, lres = V.native.VkLabelRequest(), V.VkLabelResult()
            lreq.lo, lreq.hi, lreq.connectivity = lo, math.inf, 6
            best = 1e9
            for _ in range(reps):
                t0 = time.perf_counter()
                V.native.check(ctx.handle, V.native.lib().vk_distance_transform(ctx.handle, C.byref(dreq), None, None, None, C.byref(dres)))
                V.native.check(ctx.handle, V.native.lib().vk_label_components(ctx.handle, C.byref(lreq), None, None, None, 0, None, C.byref(lres)))
                best = min(best, (time.perf_counter() - t0) * 1e3)
            out[name + "_before_ms"] = round(best, 3)
        finally:
            ctx.close()
    if vol.size <= 256 ** 3:
        import split_helpers as SH

        os.makedirs(os.path.join(HERE, "ubench", "_build"), exist_ok=True)
        L = SH.build_restatement(os.path.join(HERE, "ubench", "_build"))
        t0 = time.perf_counter()
        result = SH.restate(L, vol, "u8", lo, math.inf, 6, 3.0, cap=1)[2]
        out[vname + "_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        mine = out[f"{vname}_linear_r3_totals"]
        out[vname + "_cpu_totals_agree"] = [int(result[0]), int(result[2]), int(result[4]), int(result[6])] == mine and int(result[7]) == out[f"{vname}_linear_r3_rounds"]
    del vol
sizes = sorted({out[n + "_bytes"] for n in names})
for rep in range(reps):
    ms = stream_ms(sizes)
    for n in names:
        out[n + "_stream_ms"] = min(out.get(n + "_stream_ms", 1e9), ms[out[n + "_bytes"]])
print(json.dumps(out), flush=True)
