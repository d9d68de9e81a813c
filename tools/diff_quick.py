"""The steady-diffusion pass (vk_steady_diffusion), phase by phase, both builds of its sweep.  One row per run, so that every GPU step has a time limit of
its own:
    for row in standin standin_pores solid512 spheres512; do for part in direct lds omegas; do timeout -k 10 300 python tools/diff_quick.py --row $row --part $part || break 2; done; done
Rows (u8, PACKED; spacing 1 1 1; the Python defaults: omega automatic, check_every 32, delta_tol 1e-5, flux_tol 1e-3, max_sweeps 20000):
  standin        the 256^3 bonsai stand-in's range [0.3, inf) along z: no voxel of it lies on either face, so nothing flows and the first block converges -- what a sweep costs
  standin_pores  the stand-in's pore space (-inf, 0.3) along z: the row on which the defaults are checked
  solid512    a solid 512^3 block along x
  spheres512  the pore space (the complement) of tools/geo_quick.py's 512^3 sphere pack, from z- to z+
Per row, one part per run (--part direct | lds | omegas; a 512^3 row that does not converge costs --cap sweeps per call, so the 512^3 rows are run with --cap 4000 --reps 1).
For the sweep that loads its neighbours from global memory ("direct") and the one that stages tiles in LDS ("lds", vk_debug_set_param "diff_lds" 1):
  sweeps, converged, blocks, launches      the result and the launch counts (vk_debug_set_param "diff_timing" 9; launches come in whole batches of 4 blocks)
  <phase>_ms     each phase alone -- seed, sweeps (every block, with the checks and the host's looks at the counts), stats, dense -- between the context's timer events
                 ("diff_timing" k), best of --reps calls
  ms_per_sweep   sweeps_ms over the sweeps
  gbytes_per_s, hbm_share   the bytes a sweep must move -- the state read once and written once per colour: 4 bytes read per voxel per colour, 4 written per voxel of the set
                 per sweep -- over ms_per_sweep, and that over 8 TB/s, the MI355X's HBM3E peak
  ns_per_update  sweeps_ms over sweeps x the voxels of the set
  porosity, flux, flux_mismatch, d_eff, tau   what derives from the result
and for the direct build the sweeps to converge (capped at --cap, default 20000) with the automatic omega, with 2 - (2 - omega_auto) / 3 and with 1.0: what the choice is worth
usage: tools/diff_quick.py --row NAME --part direct|lds|omegas [--reps N] [--cap SWEEPS]"""
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
cap = int(sys.argv[sys.argv.index("--cap") + 1]) if "--cap" in sys.argv else 20000
row = sys.argv[sys.argv.index("--row") + 1]
part = sys.argv[sys.argv.index("--part") + 1]
PHASES = ((1, "seed"), (2, "sweeps"), (3, "stats"), (4, "dense"))
HBM_PEAK = 8.0e12


def spheres(n, pitch=24):
    """The sphere pack of tools/geo_quick.py and tools/split_quick.py (those are scripts and cannot be imported): centres on a jittered
    grid of pitch 24, radii 10 .. 14, the same seed, so that the rows of the three tools are the same volume."""
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


def volume():
    """(volume, lo, hi, axis)"""
    if row == "standin":
        from oracle import oracle as O

        return O.volume_standin_u8(256), 0.3, float("inf"), "z"
    if row == "standin_pores":
        from oracle import oracle as O

        return O.volume_standin_u8(256), -float("inf"), 0.3, "z"
    if row == "solid512":
        return np.full((512, 512, 512), 255, np.uint8), 0.5, float("inf"), "x"
    if row == "spheres512":
        return spheres(512), -float("inf"), 0.5, "z"
    raise SystemExit("diff_quick: --row standin | standin_pores | solid512 | spheres512")


vol, lo, hi, axis = volume()
out = {"row": row, "part": part, "voxels": int(vol.size)}
ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
try:
    V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
    res = V.native.VkDiffusionResult()
    dense = np.zeros_like(vol)

    def run(req, d=None):
        V.native.check(ctx.handle, V.native.lib().vk_steady_diffusion(ctx.handle, C.byref(req), None, None, d, C.byref(res)))
        return V.Diffusion(res, axis, tuple(reversed(vol.shape)))

    print(row, file=sys.stderr, flush=True)
    req = V.diffusion_request(lo, hi, axis=axis, max_sweeps=cap)
    for name, lds in (("direct", 0), ("lds", 1)):
        if name != part:
            continue
        ctx.set_param("diff_lds", lds)
        o = {}
        ctx.set_param("diff_timing", 9)
        t0 = time.perf_counter()
        t = run(req)
        o["first_call_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        words = V.native.lib().vk_last_error(ctx.handle).decode().split()
        o["blocks"], o["launches"] = int(words[2]), int(words[4])
        o.update(n_fg=t.n_foreground, sweeps=t.sweeps, converged=t.converged, delta=t.delta, porosity=round(t.porosity, 6), flux=t.flux, flux_mismatch=t.flux_mismatch,
                 d_eff=t.effective_diffusivity, tau=t.tortuosity_factor, omega=t.omega)
        for k, phase in PHASES:
            ctx.set_param("diff_timing", k)
            best = 1e9
            for _ in range(reps):
                run(req, dense.ctypes.data if phase == "dense" else None)
                best = min(best, ctx.timer_elapsed_ms())
            o[f"{phase}_ms"] = round(best, 4)
        ctx.set_param("diff_timing", 0)
        o["ms_per_sweep"] = round(o["sweeps_ms"] / max(t.sweeps, 1), 5)
        moved = 2 * 4 * vol.size + 4 * t.n_foreground  # per sweep: each colour's launch reads the state once; a sweep writes every voxel of the set once
        o["gbytes_per_s"] = round(moved / (o["ms_per_sweep"] * 1e-3) / 1e9, 1)
        o["hbm_share"] = round(moved / (o["ms_per_sweep"] * 1e-3) / HBM_PEAK, 4)
        o["ns_per_update"] = round(o["sweeps_ms"] * 1e6 / max(t.sweeps * t.n_foreground, 1), 5)
        out[name] = o
    ctx.set_param("diff_lds", 0)
    if part == "omegas":
        auto = run(V.diffusion_request(lo, hi, axis=axis, max_sweeps=32)).omega
        for name, w in (("auto", 0.0), ("auto_third", 2.0 - (2.0 - auto) / 3.0), ("one", 1.0)):
            t = run(V.diffusion_request(lo, hi, axis=axis, omega=w, max_sweeps=cap))
            out["omega_" + name] = {"omega": t.omega, "sweeps": t.sweeps, "converged": t.converged, "d_eff": t.effective_diffusivity}
finally:
    ctx.close()
print(json.dumps(out), flush=True)
