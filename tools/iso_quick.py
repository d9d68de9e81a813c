"""First-hit isosurface rendering on the C2 shape (256^3 bonsai stand-in, 1080p, dt 0.5, f16 out): ms per frame, one frame per launch and
128 orbit frames per launch, interleaved, best of three groups per repetition, for
  composite               the built-in transfer, composited
  max_table               VK_PROJ_MAX over the window [0.1, 1] with tools/mip_quick.py's `builtin_table`: the built-in census
  iso_air[_lit]_r{0,4}    an isosurface at 0.1, just above the stand-in's air -- a cell is empty iff its largest tap is <= 25, the census of
                          the two rows above, so the same skip policy --, unlit and under a headlight, 0 and 4 bisection steps
  iso_canopy[_lit]_r{0,4} an isosurface at 0.4, inside the canopy
The kernels refine the crossing only under lighting (unlit, neither a nor the gradient can be seen in the frame), so the unlit r4 rows run
the same kernel work as the unlit r0 rows and are there as a control: the cost of the bisection is iso_*_lit_r4 against iso_*_lit_r0, the
cost of the shade iso_*_lit_r0 against iso_*_r0.
plus every configuration's empty fraction, S_ref, S_sampled, and the frame and step checksums.  The expectation this run confirms or
refutes: at the same emptiness an unlit R = 0 frame (iso_air_r0) costs less than the MAX row, because its rays end at their first hit.
usage: tools/iso_quick.py [--reps N]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zlib

import variant

variant.use_variant_from_env()  # tools/ab.py: VK_LIB
import numpy as np
import torch

import vokselis_amd as V
from vokselis_amd import _native as N

W, H, DT, B = 1920, 1080, 0.5, 128
AIR, CANOPY = 0.1, 0.4
LIGHT = dict(direction="headlight", ambient=0.2, diffuse=0.8, specular=0.4, shininess=24.0)
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3


def builtin_table(n=256):
    """raycast_naive.wgsl:104-110 sampled at n values (tools/mip_quick.py)."""
    x = np.arange(n) / (n - 1)
    s = np.clip((np.minimum(x, 0.9) - 0.1) / 1.1, 0.0, 1.0)
    a = s * s * (3.0 - 2.0 * s)
    rgb = np.stack([0.5 + 0.5 * np.cos(6.28318 * (c * a + d)) for c, d in ((1.0, 0.0), (1.7, 0.15), (0.4, 0.20))], axis=1)
    return np.concatenate([rgb, a[:, None]], axis=1).astype(np.float32)


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


def empty_fraction(ctx):
    f = C.c_double()
    N.check(ctx.handle, N.lib().vk_volume_empty_fraction(ctx.handle, C.byref(f)))
    return f.value


cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
orbit = [V.Camera(1.0, 0.5, 1.0 + 6.28318 * j / 1024, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix() for j in range(B)]
# name, table + window + projection, isosurface (threshold, refine), lit
configs = [("composite", None, None, False), ("max_table", (builtin_table(), (0.1, 1.0)), None, False)]
for label, iso in (("air", AIR), ("canopy", CANOPY)):
    for lit in (False, True):
        for r in (0, 4):
            configs.append(("iso_%s%s_r%d" % (label, "_lit" if lit else "", r), None, (iso, r), lit))
ctxs = {}
out = {"lib": os.environ.get("VK_LIB", "product")}
for name, table, iso, lit in configs:
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
    if table is not None:
        ctx.set_transfer_function(*table)
        ctx.set_projection("max")
    if iso is not None:
        ctx.set_isosurface(iso[0], (0.9, 0.7, 0.4), iso[1])
    if lit:
        ctx.set_lighting(**LIGHT)
    V.VolumeTexture.generate_standin(ctx, (256,) * 3)
    ctx.update()
    ctx.reset_step_counts()
    V.RaycastPipeline(dt_scale=DT, flags=V.RENDER_COUNT).record(ctx)
    out[name + "_crc"] = "%08x" % zlib.crc32(ctx.read_backbuffer().tobytes())  # the frame, for A/B runs: both sides must agree
    out[name + "_steps_crc"] = "%08x" % zlib.crc32(ctx.read_steps().tobytes())
    s_ref, s_sampled = ctx.step_counts()
    out[name + "_empty_fraction"] = round(empty_fraction(ctx), 4)
    out[name + "_s_ref"], out[name + "_s_sampled"] = int(s_ref), int(s_sampled)
    ctxs[name] = ctx
frames = torch.empty((B, H, W, 4), dtype=torch.float16, device="cuda")
pipe = V.RaycastPipeline(dt_scale=DT)
for name, ctx in ctxs.items():
    for _ in range(100):
        pipe.record(ctx)
    ctx.sync()
for rep in range(reps):
    for name, ctx in ctxs.items():
        out.setdefault(name + "_single_ms", []).append(round(t(ctx, lambda: pipe.record(ctx), 50), 4))
        out.setdefault(name + "_orbit128_ms_per_frame", []).append(
            round(t(ctx, lambda: V.render_batch(ctx, pipe, orbit, frames.data_ptr(), tile_size=64), 3) / B, 5))
for k in ("single_ms", "orbit128_ms_per_frame"):
    out["iso_air_r0_over_max_table_" + k] = round(min(out["iso_air_r0_" + k]) / min(out["max_table_" + k]), 3)
    out["iso_air_r0_over_composite_" + k] = round(min(out["iso_air_r0_" + k]) / min(out["composite_" + k]), 3)
    out["iso_air_lit_r4_over_iso_air_r0_" + k] = round(min(out["iso_air_lit_r4_" + k]) / min(out["iso_air_r0_" + k]), 3)
for ctx in ctxs.values():
    ctx.close()
print(json.dumps(out), flush=True)
