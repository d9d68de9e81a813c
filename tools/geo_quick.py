"""The geodesic-distance pass (vk_geodesic_distance), phase by phase, beside the one kernel of the tree that does comparable work.  One row per run, so that
every GPU step has a time limit of its own:
    for row in standin standin_seed spheres512 solid512 serpentine512; do timeout -k 10 300 python tools/geo_quick.py --row $row || break; done
Rows (u8, PACKED; spacing 1 1 1; connectivity 26):
  standin        the 256^3 bonsai stand-in's range [0.3, inf) from the x- face (no voxel of the range lies on it: what a call costs that reaches nothing)
  standin_seed   the same range from one seed, its first voxel in raster order, to z+ (no voxel of the range lies on any face)
  spheres512     the pore space (the complement) of tools/split_quick.py's 512^3 sphere pack, from z- to z+
  solid512       a solid 512^3 block from x-: the trivial front, one sweep through the tiles
  serpentine512  a 512^3 volume whose set is slabs 6 voxels thick joined at alternating ends along y: the adversarial front, which crosses every tile column once per slab
Per row:
  <phase>_ms     each phase alone -- seed, relax (every round, with the host's looks at the counts), stats, dense -- between the context's timer events
                 (vk_debug_set_param "geo_timing" k), best of --reps calls; relax_share: relax_ms over the sum of the four
  call_ms        the blocking call end to end on the host, totals only
  rounds, launches, visits, passes, stored   the rounds that visited a tile, the relax launches (whole batches of 8), the tile visits, their LDS passes and the
                 voxel words stored (vk_debug_set_param "geo_timing" 9); passes_per_visit, stored_per_reached
  relax_ns_per_reached, relax_ns_per_update   relax_ms over the reached voxels, and over the voxel updates (passes x 4096: every pass relaxes a whole tile)
  n_fg, n_src, n_reached, max_g, target_min   the result
and with spheres512 the yardstick: vk_split_components on the sphere pack itself at radius 3 (markers survive), its growth phase alone (split_timing 3):
  split_growth_ms, split_rounds, split_ns_per_update   the growth rounds' time, their count, and the time per voxel update (launches x voxels: every round sweeps the volume)
usage: tools/geo_quick.py --row NAME [--reps N]"""
import ctypes as C
import json
import os
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
PHASES = ((1, "seed"), (2, "relax"), (3, "stats"), (4, "dense"))


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


def serpentine(n, thick=6, gap=2):
    """Slabs `thick` voxels wide along y, `gap` voxels of background between them, joined at alternating ends of x."""
    vol = np.zeros((n, n, n), np.uint8)
    left = False
    for y in range(0, n, thick + gap):
        vol[:, y:y + thick, :] = 255
        if y + thick + gap < n:
            vol[:, y + thick:y + thick + gap, 0:thick] = 255 if left else 0
            vol[:, y + thick:y + thick + gap, n - thick:n] = 0 if left else 255
        left = not left
    vol[:, n - gap:n, :] = 255  # the last slab reaches the y+ face
    return vol


def volume():
    """(volume, lo, hi, sources, targets)"""
    if row == "standin":
        from oracle import oracle as O

        return O.volume_standin_u8(256), 0.3, float("inf"), ("x-",), ("x+",)
    if row == "standin_seed":
        from oracle import oracle as O

        return O.volume_standin_u8(256), 0.3, float("inf"), (), ("z+",)
    if row == "spheres512":
        return spheres(512), -float("inf"), 0.5, ("z-",), ("z+",)
    if row == "solid512":
        return np.full((512, 512, 512), 255, np.uint8), 0.5, float("inf"), ("x-",), ("x+",)
    if row == "serpentine512":
        return serpentine(512), 0.5, float("inf"), ("y-",), ("y+",)
    raise SystemExit("geo_quick: --row standin | standin_seed | spheres512 | solid512 | serpentine512")


vol, lo, hi, sources, targets = volume()
out = {"row": row, "voxels": int(vol.size)}
ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
try:
    V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
    res = V.native.VkGeodesicResult()
    dense = np.zeros_like(vol)
    seeds = ()
    if not sources:  # the first voxel of the range in raster order
        z, y, x = np.unravel_index(int(np.argmax(vol.astype(np.float32) >= np.float32(lo) * np.float32(255.0))), vol.shape)
        seeds = ((int(x), int(y), int(z)),)
    req = V.geodesic_request(lo, hi, sources=sources, seeds=seeds, targets=targets, install=False)
    call = lambda d=None: V.native.check(ctx.handle, V.native.lib().vk_geodesic_distance(ctx.handle, C.byref(req), None, None, d, C.byref(res)))
    print(row, file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    call()
    out["first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["n_fg"], out["n_src"], out["n_reached"], out["max_g"], out["target_min"] = int(res.n_foreground), int(res.n_sources), int(res.n_reached), int(res.max_g), int(res.target_min)
    ctx.set_param("geo_timing", 9)
    call()
    words = V.native.lib().vk_last_error(ctx.handle).decode().split()
    for k in range(1, len(words) - 1, 2):
        out[words[k]] = int(words[k + 1])
    out["passes_per_visit"] = round(out["passes"] / max(out["visits"], 1), 3)
    out["stored_per_reached"] = round(out["stored"] / max(out["n_reached"], 1), 3)
    for k, phase in PHASES:
        ctx.set_param("geo_timing", k)
        best = 1e9
        for _ in range(reps):
            call(dense.ctypes.data if phase == "dense" else None)
            best = min(best, ctx.timer_elapsed_ms())
        out[f"{phase}_ms"] = round(best, 4)
    ctx.set_param("geo_timing", 0)
    out["relax_share"] = round(out["relax_ms"] / sum(out[f"{p}_ms"] for _, p in PHASES), 4)
    out["relax_ns_per_reached"] = round(out["relax_ms"] * 1e6 / max(out["n_reached"], 1), 3)
    out["relax_ns_per_update"] = round(out["relax_ms"] * 1e6 / max(out["passes"] * 4096, 1), 4)
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    out["call_ms"] = round(best, 3)
    if row == "spheres512":  # the yardstick: the split pass's whole-volume growth rounds on the spheres themselves
        sreq = V.split_request(0.5, radius=3.0)
        sres = V.native.VkSplitResult()
        split = lambda: V.native.check(ctx.handle, V.native.lib().vk_split_components(ctx.handle, C.byref(sreq), None, None, None, 0, None, C.byref(sres)))
        ctx.set_param("split_timing", 3)
        best = 1e9
        for _ in range(reps):
            split()
            best = min(best, ctx.timer_elapsed_ms())
        ctx.set_param("split_timing", 0)
        launches = (int(sres.rounds) // 8 + 1) * 8
        out["split_growth_ms"], out["split_rounds"], out["split_markers"] = round(best, 4), int(sres.rounds), int(sres.n_markers)
        out["split_ns_per_update"] = round(best * 1e6 / (launches * vol.size), 5)
finally:
    ctx.close()
print(json.dumps(out), flush=True)
