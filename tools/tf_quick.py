"""The runtime transfer function on the C2 shape (256^3 bonsai stand-in, 1080p, dt 0.5): ms per frame of the built-in transfer against two
tables with its zero band (alpha 0 below 0.1: the same census, so the same skip policy) -- `table`: the tests' zero-band table, more
transparent than the built-in, so its rays sample more steps; `builtin_table`: the built-in transfer and palette sampled into 256
entries, whose rays sample (nearly) the built-in's steps -- one frame per launch and 128 orbit frames per launch, interleaved, best of
three groups per repetition; plus every table's empty fraction, sampled steps, and its cost per sampled step against the built-in's.
usage: tools/tf_quick.py [--reps N]"""
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

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from tf_helpers import zero_band_table  # noqa: E402

W, H, DT, B = 1920, 1080, 0.5, 128
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3


def builtin_table(n=256):
    """raycast_naive.wgsl:104-110 sampled at n values: alpha = smoothstep(0.1, 1.2, min(v, 0.9)), colour = the vertigo palette of alpha."""
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
tables = [("builtin", None), ("table", zero_band_table()), ("builtin_table", builtin_table())]
ctxs = {}
out = {"lib": os.environ.get("VK_LIB", "product")}
for name, table in tables:
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
    if table is not None:
        ctx.set_transfer_function(table)
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
    for _ in range(200):
        pipe.record(ctx)
    ctx.sync()
for rep in range(reps):
    for name, ctx in ctxs.items():
        out.setdefault(name + "_single_ms", []).append(round(t(ctx, lambda: pipe.record(ctx), 50), 4))
        out.setdefault(name + "_orbit128_ms_per_frame", []).append(
            round(t(ctx, lambda: V.render_batch(ctx, pipe, orbit, frames.data_ptr(), tile_size=64), 3) / B, 5))
for tname in ("table", "builtin_table"):
    steps = out[tname + "_s_sampled"] / out["builtin_s_sampled"]
    for name in ("single_ms", "orbit128_ms_per_frame"):
        r = min(out[tname + "_" + name]) / min(out["builtin_" + name])
        out[tname + "_over_builtin_" + name] = round(r, 3)
        out[tname + "_over_builtin_per_sampled_step_" + name] = round(r / steps, 3)
for ctx in ctxs.values():
    ctx.close()
print(json.dumps(out), flush=True)
