"""The local-thickness pass (vk_local_thickness), phase by phase, beside its yardsticks.  One row per run, so that
every GPU step has a time limit of its own:
    for row in standin solid256 spheres512 solid512; do timeout -k 10 300 python tools/thick_quick.py --row $row || break; done
Rows (u8, PACKED; spacing 1 1 1):
  standin      the 256^3 bonsai stand-in at the threshold 0.3, cap 8, 16 and 32
  spheres512   the 512^3 sphere pack of tools/split_quick.py, cap 16
  solid256     the worst case by construction: a solid block inside a margin of 16 voxels, 256^3, cap 8, 16 and 32 -- the tiles of its
               shell see a full window of saturated tiles
  solid512     the same at 512^3 (run it only when solid256 says it is safe under the limit)
Per row and cap:
  <phase>_ms   each phase alone -- distance (the borrowed kernels), tile_max, gather, stats, dense -- between the context's timer
               events (vk_debug_set_param "thick_timing" k), best of --reps calls
  call_ms      the blocking call end to end on the host, totals only
  inside_ms    vk_distance_transform(VK_DIST_INSIDE), result only, in the same run: what the call costs before the new kernels
  n_fg, max_t2, n_sat, mean_t2   the result
  with --count (tools/thick_evals.cpp, the kernel's walk replayed on the host's CPUs over the library's own distance array):
  pairs_tested, pairs_accepted, entries, evals   the tile pairs the walk tested and accepted, the centres kept over all accepted pairs,
               and the centre evaluations (entries x 512 threads); replay_differs: the voxels where the replay's T2 is not the library's (0)
and per row
  stream_ms    a sum over an array of one word per voxel with 16-byte loads (tools/ubench/stream_read.hip): tools/dist_quick.py's yardstick
usage: tools/thick_quick.py --row NAME [--reps N] [--count]"""
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
row = sys.argv[sys.argv.index("--row") + 1]
PHASES = ((1, "distance"), (2, "tile_max"), (3, "gather"), (4, "stats"), (5, "dense"))


def stream_ms(sizes):
    src, exe = os.path.join(HERE, "ubench", "stream_read.hip"), os.path.join(HERE, "ubench", "_build", "stream_read")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    r = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=300)
    return {int(k): v for k, v in json.loads(r.stdout).items()}


def counter():
    so = os.path.join(HERE, "ubench", "_build", "libthick_evals.so")
    src = os.path.join(HERE, "thick_evals.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-fopenmp", "-shared", "-fPIC", "-I", os.path.join(ROOT, "vokselis_amd", "csrc"), "-o", so, src], check=True)
    L = C.CDLL(so)
    L.thick_count.restype = C.c_uint64
    return L


def spheres(n, pitch=24):
    """tools/split_quick.py's pack: centres on a jittered grid of pitch 24, radii 10 .. 14, so that neighbours touch."""
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


def solid(n, margin=16):
    vol = np.zeros((n, n, n), np.uint8)
    vol[margin:n - margin, margin:n - margin, margin:n - margin] = 255
    return vol


def volume():
    if row == "standin":
        from oracle import oracle as O

        return O.volume_standin_u8(256), 0.3, (8.0, 16.0, 32.0)
    if row == "spheres512":
        return spheres(512), 0.5, (16.0,)
    if row in ("solid256", "solid512"):
        return solid(int(row[5:])), 0.5, (8.0, 16.0, 32.0)
    raise SystemExit("thick_quick: --row standin | spheres512 | solid256 | solid512")


vol, lo, caps = volume()
out = {"row": row, "voxels": int(vol.size)}
ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
try:
    V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
    res = V.native.VkThicknessResult()
    dense = np.zeros_like(vol)
    for cap in caps:
        name = "cap%d" % int(cap)
        print(row, name, file=sys.stderr, flush=True)
        req = V.thickness_request(lo, max_radius=cap)
        call = lambda d=None: V.native.check(ctx.handle, V.native.lib().vk_local_thickness(ctx.handle, C.byref(req), None, None, d, C.byref(res)))
        t0 = time.perf_counter()
        call()
        out[name + "_first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        out[name + "_n_fg"], out[name + "_max_t2"], out[name + "_n_sat"] = int(res.n_foreground), int(res.max_t2), int(res.n_saturated)
        out[name + "_mean_t2"] = round(int(res.sum_t2) / max(int(res.n_foreground), 1), 3)
        for k, phase in PHASES:
            ctx.set_param("thick_timing", k)
            best = 1e9
            for _ in range(reps):
                call(dense.ctypes.data if phase == "dense" else None)
                best = min(best, ctx.timer_elapsed_ms())
            out[f"{name}_{phase}_ms"] = round(best, 4)
        ctx.set_param("thick_timing", 0)
        best = 1e9
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        out[name + "_call_ms"] = round(best, 3)
        if "--count" in sys.argv and cap <= 16.0:  # (cap 32 on the solid block is minutes of CPU)
            d2, t2 = np.zeros(vol.shape, np.uint32), np.zeros(vol.shape, np.uint32)
            inside = V.distance_request(lo, op="inside")
            V.native.check(ctx.handle, V.native.lib().vk_distance_transform(ctx.handle, C.byref(inside), None, d2.ctypes.data, None, None))
            V.native.check(ctx.handle, V.native.lib().vk_local_thickness(ctx.handle, C.byref(req), None, t2.ctypes.data, None, None))
            counts, w = np.zeros(5, np.uint64), np.ones(3, np.uint32)
            nz, ny, nx = vol.shape
            out[name + "_replay_differs"] = int(counter().thick_count(C.c_void_p(d2.ctypes.data), C.c_void_p(t2.ctypes.data), C.c_uint32(nx), C.c_uint32(ny), C.c_uint32(nz),
                                                                     C.c_void_p(w.ctypes.data), C.c_uint32(int(cap * cap)), C.c_void_p(counts.ctypes.data)))
            for k, word in enumerate(("pairs_tested", "pairs_accepted", "entries", "evals", "tiles_walking")):
                out[f"{name}_{word}"] = int(counts[k])
    inside = V.distance_request(lo, op="inside")
    dres = V.native.VkDistanceResult()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        V.native.check(ctx.handle, V.native.lib().vk_distance_transform(ctx.handle, C.byref(inside), None, None, None, C.byref(dres)))
        best = min(best, (time.perf_counter() - t0) * 1e3)
    out["inside_ms"] = round(best, 3)
    out["max_d2"] = int(dres.max_d2)
finally:
    ctx.close()
words = vol.size * 4
out["stream_ms"] = min(stream_ms([words])[words] for _ in range(reps))
print(json.dumps(out), flush=True)
