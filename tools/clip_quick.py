"""What a clip box (vk_set_clip_box) buys on the C2 shape (256^3 bonsai stand-in, 1080p, dt 0.5, f16 out) under tools/mip_quick.py's
`builtin_table`: ms per frame, one frame per launch and 128 orbit frames per launch, interleaved, best of three groups per repetition, for
  none    no box
  unit    the box (0, 0, 0) - (1, 1, 1): the frame and the steps of `none`, bit for bit (asserted)
  half    the half-space (0.5, 0, 0) - (1, 1, 1)
  roi     the region of interest (0.25, 0.3, 0.1) - (0.8, 0.75, 0.6)
each for the table march and the first-hit isosurface at 0.4 under a headlight, plus every configuration's S_ref, S_sampled, active
64-pixel tiles (vk_partition_active) and the frame and step checksums.
usage: tools/clip_quick.py [--reps N]"""
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

W, H, DT, B = 1920, 1080, 0.5, 128
BOXES = (("none", None), ("unit", ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))), ("half", ((0.5, 0.0, 0.0), (1.0, 1.0, 1.0))),
         ("roi", ((0.25, 0.3, 0.1), (0.8, 0.75, 0.6))))
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


cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
orbit = [V.Camera(1.0, 0.5, 1.0 + 6.28318 * j / 1024, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix() for j in range(B)]
ctxs = {}
out = {"lib": os.environ.get("VK_LIB", "product")}
for family in ("table", "iso"):
    for label, box in BOXES:
        name = family + "_" + label
        ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
        if family == "table":
            ctx.set_transfer_function(builtin_table())
        else:
            ctx.set_isosurface(0.4, (0.9, 0.7, 0.4), 4)
            ctx.set_lighting(**LIGHT)
        if box is not None:
            ctx.set_clip_box(*box)
        V.VolumeTexture.generate_standin(ctx, (256,) * 3)
        ctx.update()
        ctx.reset_step_counts()
        V.RaycastPipeline(dt_scale=DT, flags=V.RENDER_COUNT).record(ctx)
        out[name + "_crc"] = "%08x" % zlib.crc32(ctx.read_backbuffer().tobytes())  # the frame, for A/B runs: both sides must agree
        out[name + "_steps_crc"] = "%08x" % zlib.crc32(ctx.read_steps().tobytes())
        s_ref, s_sampled = ctx.step_counts()
        out[name + "_s_ref"], out[name + "_s_sampled"] = int(s_ref), int(s_sampled)
        out[name + "_active_tiles"] = ctx.partition_active(64)[0]
        ctxs[name] = ctx
    assert out[family + "_unit_crc"] == out[family + "_none_crc"] and out[family + "_unit_steps_crc"] == out[family + "_none_steps_crc"], "the unit box is not no box"
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
for family in ("table", "iso"):
    for k in ("single_ms", "orbit128_ms_per_frame"):
        for label in ("unit", "half", "roi"):
            out["%s_%s_over_none_%s" % (family, label, k)] = round(min(out["%s_%s_%s" % (family, label, k)]) / min(out["%s_none_%s" % (family, k)]), 3)
for ctx in ctxs.values():
    ctx.close()
print(json.dumps(out), flush=True)
