"""Gradient lighting on the C2 shape (256^3 bonsai stand-in, 1080p, dt 0.5) with tools/tf_quick.py's `builtin_table` (the built-in transfer
and palette sampled into 256 entries): ms per frame of the unlit table against a headlight and against a fixed world light, one frame per
launch and 128 orbit frames per launch, interleaved, best of three groups per repetition.  Lighting leaves alpha alone, so every variant
samples the same steps (checked): the ratios are the cost per sampled step of the shade.
usage: tools/lit_quick.py [--reps N]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zlib

import variant

variant.use_variant_from_env()  # tools/ab.py: VK_LIB
import torch

import vokselis_amd as V

W, H, DT, B = 1920, 1080, 0.5, 128
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3


def builtin_table(n=256):
    """tools/tf_quick.py: builtin_table (repeated here: that script runs its measurement when imported)."""
    import numpy as np

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
variants = [("unlit", None), ("headlight", dict(direction="headlight")), ("world", dict(direction=(0.4, -0.8, 0.45), ambient=0.1, diffuse=0.9, specular=0.6, shininess=64.0))]
ctxs = {}
out = {"lib": os.environ.get("VK_LIB", "product")}
for name, light in variants:
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
    ctx.set_transfer_function(builtin_table())
    if light is not None:
        ctx.set_lighting(**light)
    V.VolumeTexture.generate_standin(ctx, (256,) * 3)
    ctx.update()
    ctx.reset_step_counts()
    V.RaycastPipeline(dt_scale=DT, flags=V.RENDER_COUNT).record(ctx)
    out[name + "_crc"] = "%08x" % zlib.crc32(ctx.read_backbuffer().tobytes())  # the frame, for A/B runs: both sides must agree
    out[name + "_steps_crc"] = "%08x" % zlib.crc32(ctx.read_steps().tobytes())
    out[name + "_s_ref"], out[name + "_s_sampled"] = (int(v) for v in ctx.step_counts())
    ctxs[name] = ctx
assert len({out[n + "_s_sampled"] for n, _ in variants}) == 1, out  # lighting never changes the steps
frames = torch.empty((B, H, W, 4), dtype=torch.float16, device="cuda")
pipe = V.RaycastPipeline(dt_scale=DT)
for name, ctx in ctxs.items():
    for _ in range(200):
        pipe.record(ctx)
    ctx.sync()
for rep in range(reps):
    for name, ctx in ctxs.items():
        out.setdefault(name + "_single_ms", []).append(round(t(ctx, lambda: pipe.record(ctx), 50), 4))
        out.setdefault(name + "_orbit128_ms_per_frame", []).append(
            round(t(ctx, lambda: V.render_batch(ctx, pipe, orbit, frames.data_ptr(), tile_size=64), 3) / B, 5))
for name in ("headlight", "world"):
    for m in ("single_ms", "orbit128_ms_per_frame"):
        out[name + "_over_unlit_" + m] = round(min(out[name + "_" + m]) / min(out["unlit_" + m]), 3)
for ctx in ctxs.values():
    ctx.close()
print(json.dumps(out), flush=True)
