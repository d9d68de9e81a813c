"""R16_UNORM volumes on the C2 shape (256^3 bonsai stand-in, 1080p, dt 0.5, f16 out): ms per frame of the built-in transfer and of the
built-in transfer sampled into a 256-entry table (`builtin_table`, tools/tf_quick.py's), one frame per launch and 128 orbit frames per
launch, for the same values in three formats --
    u8     the stand-in itself, PACKED and PACKED_PAIRS
    u16    its x257 widening (v * 257 / 65535 = v / 255), PACKED
    f16    the same values v / 255 rounded to f16, PACKED: the yardstick, the same cell bytes and within two instructions per sample
-- interleaved, best of three groups per repetition; with every row's empty fraction, S_ref, S_sampled and checksums.  The u16 and u8
rows march the same steps (the widening is exact); the f16 row's values are rounded, so its steps differ a little.
usage: tools/u16_quick.py [--reps N] [--no-u16]     (--no-u16: the rows a library without the format has -- VK_LIB=<the parent's>)"""
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
from vokselis_amd import volumes

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


u8 = np.ascontiguousarray(volumes.bonsai_standin(256))  # (bit-identical to the device generator's)
vols = [("u8_packed", u8, V.LAYOUT_PACKED, None), ("u8_pairs", u8, V.LAYOUT_PACKED_PAIRS, None),
        ("f16_packed", (u8.astype(np.float64) / 255.0).astype(np.float16), V.LAYOUT_PACKED, None)]
if "--no-u16" not in sys.argv:
    vols.insert(2, ("u16_packed", u8.astype(np.uint16) * np.uint16(257), V.LAYOUT_PACKED, V.FMT_R16_UNORM))
cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
orbit = [V.Camera(1.0, 0.5, 1.0 + 6.28318 * j / 1024, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix() for j in range(B)]
out = {"lib": os.environ.get("VK_LIB", "product")}
ctxs = {}
for vname, vol, layout, fmt in vols:
    for tname, table in (("builtin", None), ("builtin_table", builtin_table())):
        name = vname + "." + tname
        ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
        if table is not None:
            ctx.set_transfer_function(table)
        if fmt is None:
            V.VolumeTexture(ctx, vol, layout=layout)
        else:
            V.VolumeTexture(ctx, vol, layout=layout, fmt=fmt)
        ctx.update()
        ctx.reset_step_counts()
        V.RaycastPipeline(dt_scale=DT, flags=V.RENDER_COUNT).record(ctx)
        out[name + "_crc"] = "%08x" % zlib.crc32(ctx.read_backbuffer().tobytes())
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
if "u16_packed.builtin" in ctxs:
    for tname in ("builtin", "builtin_table"):
        for name in ("single_ms", "orbit128_ms_per_frame"):
            for other in ("f16_packed", "u8_packed", "u8_pairs"):
                out["u16_over_%s.%s_%s" % (other, tname, name)] = round(min(out["u16_packed.%s_%s" % (tname, name)]) / min(out["%s.%s_%s" % (other, tname, name)]), 3)
for ctx in ctxs.values():
    ctx.close()
print(json.dumps(out), flush=True)
