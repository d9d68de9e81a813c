"""The skeleton pass (vk_skeletonize), phase by phase, beside two yardsticks from the same run.  One row per run, so that every GPU step has a
time limit of its own:
    for row in standin spheres512 pores512 solid512; do timeout -k 10 300 python tools/skel_quick.py --row $row || break; done
Rows (u8, PACKED; curve mode, to convergence):
  standin     the 256^3 bonsai stand-in's range [0.3, inf)
  spheres512  tools/split_quick.py's 512^3 sphere pack, the spheres themselves
  pores512    ... its pore space (the complement)
  solid512    a solid 512^3 block: the worst case, 256 iterations, one voxel layer per iteration
Per row:
  <phase>_ms     each phase alone -- seed, thin (every sub-pass of every iteration, with the host's looks at the counts), stats, dense -- between the context's timer
                 events (vk_debug_set_param "skel_timing" k), best of --reps calls; thin_share: thin_ms over the sum of the four
  call_ms        the blocking call end to end on the host, totals only
  iterations, launches, visits, deleted   the iterations that deleted something, the thin launches (eight per iteration, whole batches of four iterations), the tile
                 visits of those launches and the voxels deleted (vk_debug_set_param "skel_timing" 9); visits_per_launch, idle_share (the workgroups that found
                 their tile unstamped, over all launched)
  thin_ns_per_deleted, thin_us_per_launch   thin_ms over the voxels deleted, and over the launches
  n_fg, n_skel, n_end, n_junction   the result
and the two yardsticks:
  stream_ms, stream_all_launches_ms   one streaming read of the state bytes (one per voxel; tools/ubench/stream_read.hip, built on first use and run as a child of this
                 run), and that times the launches: what the thin phase would cost if every launch read the whole state once and did nothing else
  erode_ms       vk_morph_volume "erode" at radius 1 on the same set, the call between two events: the pass of the tree that peels one layer without preserving topology
usage: tools/skel_quick.py --row NAME [--reps N]"""
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
PHASES = ((1, "seed"), (2, "thin"), (3, "stats"), (4, "dense"))


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


def stream_ms(sizes):
    """{bytes: ms} from the streaming-read micro-benchmark."""
    src, exe = os.path.join(HERE, "ubench", "stream_read.hip"), os.path.join(HERE, "ubench", "_build", "stream_read")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    r = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=300)
    return {int(k): v for k, v in json.loads(r.stdout).items()}


def volume():
    """(volume, lo, hi)"""
    if row == "standin":
        from oracle import oracle as O

        return O.volume_standin_u8(256), 0.3, float("inf")
    if row == "spheres512":
        return spheres(512), 0.5, float("inf")
    if row == "pores512":
        return spheres(512), -float("inf"), 0.5
    if row == "solid512":
        return np.full((512, 512, 512), 255, np.uint8), 0.5, float("inf")
    raise SystemExit("skel_quick: --row standin | spheres512 | pores512 | solid512")


vol, lo, hi = volume()
out = {"row": row, "voxels": int(vol.size)}
out["stream_ms"] = round(stream_ms([vol.size])[vol.size], 4)  # the child process ends before this one opens the device
ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
try:
    V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
    res = V.native.VkSkeletonResult()
    dense = np.zeros_like(vol)
    req = V.skeleton_request(lo, hi, install=False)
    call = lambda d=None: V.native.check(ctx.handle, V.native.lib().vk_skeletonize(ctx.handle, C.byref(req), None, None, d, C.byref(res)))
    print(row, file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    call()
    out["first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["n_fg"], out["n_skel"], out["n_end"], out["n_junction"], out["converged"] = int(res.n_foreground), int(res.n_skeleton), int(res.n_end), int(res.n_junction), int(res.converged)
    ctx.set_param("skel_timing", 9)
    call()
    words = V.native.lib().vk_last_error(ctx.handle).decode().split()
    for k in range(1, len(words) - 1, 2):
        out[words[k]] = int(words[k + 1])
    tiles = ((vol.shape[2] + 31) // 32) * ((vol.shape[1] + 15) // 16) * ((vol.shape[0] + 7) // 8)
    out["visits_per_launch"] = round(out["visits"] / max(out["launches"], 1), 2)
    out["idle_share"] = round(1.0 - out["visits"] / max(out["launches"] * tiles, 1), 4)
    for k, phase in PHASES:
        ctx.set_param("skel_timing", k)
        best = 1e9
        for _ in range(reps):
            call(dense.ctypes.data if phase == "dense" else None)
            best = min(best, ctx.timer_elapsed_ms())
        out[f"{phase}_ms"] = round(best, 4)
    ctx.set_param("skel_timing", 0)
    out["thin_share"] = round(out["thin_ms"] / sum(out[f"{p}_ms"] for _, p in PHASES), 4)
    out["thin_ns_per_deleted"] = round(out["thin_ms"] * 1e6 / max(out["deleted"], 1), 3)
    out["thin_us_per_launch"] = round(out["thin_ms"] * 1e3 / max(out["launches"], 1), 3)
    out["stream_all_launches_ms"] = round(out["stream_ms"] * out["launches"], 3)
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    out["call_ms"] = round(best, 3)
    best = 1e9
    for _ in range(reps):  # the yardstick: one erosion of the same set
        ctx.timer_begin()
        ctx.morph_volume(lo, hi, op="erode", radius=1.0, install=False)
        ctx.timer_end()
        best = min(best, ctx.timer_elapsed_ms())
    out["erode_ms"] = round(best, 4)
finally:
    ctx.close()
print(json.dumps(out), flush=True)
