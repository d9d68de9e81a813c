"""The geometry pass of the first-hit isosurface on the C2 shape (256^3 bonsai stand-in, 1080p, dt 0.5, R = 4): ms per frame, one frame per
launch, interleaved, best of three groups per repetition, at iso 0.1 (just above the stand-in's air) and iso 0.4 (inside the canopy), for
  geom          the geometry pass alone (vk_render_geometry)
  colour_lit    the lit R = 4 colour render alone (f16 out): the frame whose ray, loops and bisection the pass repeats
  both          the colour render, then the geometry pass, in sequence on one stream: colour and geometry of the same frame
  pick_ms       vk_pick end to end at the frame's centre: a launch of one wave, a 32-byte download and the host's wait
plus the hit count and the surface's checksum.  The expectation this run confirms or refutes: the pass costs about the lit R = 4 colour
frame plus 32 bytes per pixel of stores (66 MB at 1080p: on the order of 10 us at HBM rates).
usage: tools/geom_quick.py [--reps N]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zlib

import variant

variant.use_variant_from_env()  # tools/ab.py: VK_LIB
import numpy as np
import torch  # noqa: F401  (one HIP runtime per process: before the library)

import vokselis_amd as V

W, H, DT, R = 1920, 1080, 0.5, 4
LIGHT = dict(direction="headlight", ambient=0.2, diffuse=0.8, specular=0.4, shininess=24.0)
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3


def t(ctx, fn, iters, groups=3):
    for _ in range(2):
        fn()
    ctx.sync()
    best = 1e9
    for _ in range(groups):
        ctx.timer_begin()
        for _ in range(iters):
            fn()
        ctx.timer_end()
        best = min(best, ctx.timer_elapsed_ms() / iters)
    return best


def wall(fn, iters, groups=3):
    best = 1e9
    for _ in range(groups):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        best = min(best, (time.perf_counter() - t0) * 1e3 / iters)
    return best


cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
ctxs = {}
out = {"lib": os.environ.get("VK_LIB", "product")}
for label, iso in (("air", 0.1), ("canopy", 0.4)):
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
    ctx.set_isosurface(iso, (0.9, 0.7, 0.4), R)
    ctx.set_lighting(**LIGHT)
    V.VolumeTexture.generate_standin(ctx, (256,) * 3)
    ctx.update()
    ctx.render_geometry(DT)
    pos_t, grad_x = ctx.read_geometry()
    out[label + "_hits"] = int(np.isfinite(pos_t[..., 3]).sum())
    out[label + "_crc"] = "%08x" % zlib.crc32(np.stack([pos_t, grad_x], axis=2).tobytes())  # the surface, for A/B runs: both sides must agree
    ctxs[label] = ctx
pipe = V.RaycastPipeline(dt_scale=DT)
for ctx in ctxs.values():
    for _ in range(100):
        pipe.record(ctx)
        ctx.render_geometry(DT)
    ctx.sync()


def both(ctx):
    pipe.record(ctx)
    ctx.render_geometry(DT)


for rep in range(reps):
    for label, ctx in ctxs.items():
        out.setdefault(label + "_geom_ms", []).append(round(t(ctx, lambda: ctx.render_geometry(DT), 50), 4))
        out.setdefault(label + "_colour_lit_ms", []).append(round(t(ctx, lambda: pipe.record(ctx), 50), 4))
        out.setdefault(label + "_both_ms", []).append(round(t(ctx, lambda: both(ctx), 50), 4))
        out.setdefault(label + "_pick_ms", []).append(round(wall(lambda: ctx.pick(W // 2, H // 2, DT), 200), 4))
for label in ctxs:
    out[label + "_geom_over_colour_lit"] = round(min(out[label + "_geom_ms"]) / min(out[label + "_colour_lit_ms"]), 3)
    out[label + "_geom_minus_colour_lit_us"] = round(1e3 * (min(out[label + "_geom_ms"]) - min(out[label + "_colour_lit_ms"])), 1)
for ctx in ctxs.values():
    ctx.close()
print(json.dumps(out), flush=True)
