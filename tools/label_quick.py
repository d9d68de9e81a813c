"""The connected-components pass (vk_label_components), kernel by kernel, beside two yardsticks.  Volumes, u8, LINEAR
and PACKED each:
  standin      the 256^3 bonsai stand-in at the threshold 0.3
  perc512      a 512^3 site-percolation field at density 79 / 256 = 0.309, the cubic lattice's threshold: the worst case for seams
  perc1024     the same at 1024^3
Per volume, layout and connectivity (6, 26):
  <phase>_ms   each of the seven kernels alone -- tile, seam, flatten, scan, number, label, mask -- between the context's timer events
               (vk_debug_set_param "label_timing" k), best of --reps calls; the calls ask for the totals only (mask: for dense_out)
  call_ms      the blocking call end to end on the host, totals only, and keep_ms with KEEP_LARGEST 1 into dense_out
  n, n_fg      components and foreground voxels
and per volume and layout
  stream_ms    a sum over the layout's array with 16-byte loads (tools/ubench/stream_read.hip, as tools/filter_quick.py runs it)
  cpu_ms       the C restatement (tests/label_restatement.c, gcc -O2, one thread) on the same dense volume at connectivity 6 -- not for
               1024^3 -- with its totals, which must be the library's
usage: tools/label_quick.py [--reps N] [--small]   (--small: no 1024^3)"""
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
PHASES = ("tile", "seam", "flatten", "scan", "number", "label", "mask")


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


def restatement():
    import label_helpers as LH

    os.makedirs(os.path.join(HERE, "ubench", "_build"), exist_ok=True)
    return LH, LH.build_restatement(os.path.join(HERE, "ubench", "_build"))


out = {}
names = []
for vname, vol, lo in volumes():
    dims = tuple(reversed(vol.shape))
    for layout, lname in ((V.LAYOUT_LINEAR, "linear"), (V.LAYOUT_PACKED, "packed")):
        name = f"{vname}_{lname}"
        names.append(name)
        out[name + "_bytes"] = vol.size if layout == V.LAYOUT_LINEAR else cell_bytes(dims, 8)
        ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
        try:
            V.VolumeTexture(ctx, vol, layout=layout)
            dense = np.zeros_like(vol)
            for conn in (6, 26):
                key = f"{name}_c{conn}"
                req = V.native.VkLabelRequest()
                req.lo, req.hi, req.connectivity = lo, math.inf, conn
                res = V.native.VkLabelResult()
                call = lambda d=None: V.native.check(ctx.handle, V.native.lib().vk_label_components(ctx.handle, C.byref(req), None, None, None, 0, d, C.byref(res)))
                call()
                out[key + "_n"], out[key + "_n_fg"] = int(res.n_components), int(res.n_foreground)
                for k, phase in enumerate(PHASES, 1):
                    ctx.set_param("label_timing", k)
                    best = 1e9
                    for _ in range(reps):
                        call(dense.ctypes.data if phase == "mask" else None)
                        best = min(best, ctx.timer_elapsed_ms())
                    out[f"{key}_{phase}_ms"] = round(best, 4)
                ctx.set_param("label_timing", 0)
                out[key + "_kernels_ms"] = round(sum(out[f"{key}_{p}_ms"] for p in PHASES), 4)
                best = 1e9
                for _ in range(reps):
                    t0 = time.perf_counter()
                    call()
                    best = min(best, (time.perf_counter() - t0) * 1e3)
                out[key + "_call_ms"] = round(best, 3)
                req.keep, req.count = V.LABEL_KEEP_LARGEST, 1
                t0 = time.perf_counter()
                call(dense.ctypes.data)
                out[key + "_keep_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                out[key + "_kept_voxels"] = int(res.n_kept_voxels)
        finally:
            ctx.close()
    if vol.size <= 512 ** 3:
        LH, L = restatement()
        t0 = time.perf_counter()
        _, _, result, _ = LH.restate(L, vol, "u8", lo, math.inf, 6, cap=1)
        out[vname + "_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out[vname + "_cpu_totals_agree"] = [int(result[0]), int(result[1])] == [out[f"{vname}_linear_c6_n"], out[f"{vname}_linear_c6_n_fg"]]
    del vol
sizes = sorted({out[n + "_bytes"] for n in names})
for rep in range(reps):
    ms = stream_ms(sizes)
    for n in names:
        out[n + "_stream_ms"] = min(out.get(n + "_stream_ms", 1e9), ms[out[n + "_bytes"]])
print(json.dumps(out), flush=True)
