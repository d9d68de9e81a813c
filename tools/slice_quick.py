"""The slice pass (vk_render_slice) at 1080p, rgba16f out: ms per frame, one launch per frame, interleaved, best of
three groups per repetition, for
  standin   the 256^3 bonsai stand-in, u8 PACKED_PAIRS
  ct        a 512 x 512 x 300 R16_UNORM volume (smooth shells plus noise), PACKED
each under an axial plane (facing z, the cube filling the frame's height) and an oblique one (normal (1, 1, 1)), with
  s1 / s1_values     one sample per pixel, without and with the value surface
  s16 / s64          a MEAN slab of 16 / 64 samples over a tenth of the cube
plus the inside pixels, the frame's checksum (for A/B runs: both sides must agree) and
  probe_ms           vk_slice_probe end to end at the frame's centre: a launch of one wave, an 8-byte download and the host's wait.
The expectation this run confirms or refutes is written in DESIGN.md section 19 before the run: one sample per pixel is bound by its stores
and one cell fetch per pixel over the HBM rate plus the launch; a slab sample costs the instruction count read from the ISA.
usage: tools/slice_quick.py [--reps N]"""
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

W, H = 1920, 1080
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


def ct_volume():
    nx, ny, nz = 512, 512, 300
    z, y, x = np.linspace(-1, 1, nz, dtype=np.float32)[:, None, None], np.linspace(-1, 1, ny, dtype=np.float32)[None, :, None], np.linspace(-1, 1, nx, dtype=np.float32)[None, None, :]
    r = np.sqrt(x * x + y * y + 0.6 * z * z)
    v = 1000.0 + 1200.0 * (r < 0.8) + 1800.0 * ((r > 0.7) & (r < 0.8)) + 300.0 * np.sin(9.0 * x) * np.cos(7.0 * y)
    v = v + np.random.default_rng(5).integers(0, 60, v.shape).astype(np.float32)
    return np.clip(v, 0, 65535).astype(np.uint16)


def planes(dims, samples):
    kw = dict(samples=samples, reduce="mean", thickness=0.1 if samples > 1 else 0.0, dims=dims)
    return {"axial": V.Slice.plane((0.5, 0.5, 0.5), (0, 0, 1), (0, 1, 0), W, H, W / H, **kw),
            "oblique": V.Slice.plane((0.5, 0.5, 0.5), (1, 1, 1), (0, 0, 1), W, H, 1.6 * W / H, **kw)}


ctxs = {}
out = {"lib": os.environ.get("VK_LIB", "product")}
ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
V.VolumeTexture.generate_standin(ctx, (256,) * 3, layout=V.LAYOUT_PACKED_PAIRS)
ctxs["standin"] = (ctx, (256, 256, 256))
ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
ctx.set_transfer_function(np.linspace(0.0, 1.0, 256 * 4, dtype=np.float32).reshape(256, 4), (900.0 / 65535.0, 4200.0 / 65535.0))  # a CT window
V.VolumeTexture(ctx, ct_volume(), layout=V.LAYOUT_PACKED, fmt=V.FMT_R16_UNORM)
ctxs["ct"] = (ctx, (512, 512, 300))

runs = []
for vname, (ctx, dims) in ctxs.items():
    for samples, tag in ((1, "s1"), (16, "s16"), (64, "s64")):
        for pname, s in planes(dims, samples).items():
            ctx.render_slice(s, values=True)
            val = ctx.read_slice_values()
            key = f"{vname}_{pname}_{tag}"
            out[key + "_inside"] = int((val[..., 1] != 0).sum())
            out[key + "_crc"] = "%08x" % zlib.crc32(ctx.read_backbuffer().tobytes() + val.tobytes())
            runs.append((key, ctx, s, False))
            if samples == 1:
                runs.append((key + "_values", ctx, s, True))
for _, ctx, s, values in runs:  # warm: clocks, caches, the allocator
    for _ in range(20):
        ctx.render_slice(s, values=values)
    ctx.sync()
for rep in range(reps):
    for key, ctx, s, values in runs:
        out.setdefault(key + "_ms", []).append(round(t(ctx, lambda: ctx.render_slice(s, values=values), 50), 4))
    for vname, (ctx, dims) in ctxs.items():
        s = planes(dims, 1)["oblique"]
        out.setdefault(vname + "_probe_ms", []).append(round(wall(lambda: ctx.slice_probe(s, W // 2, H // 2), 200), 4))
for key in [k for k in out if k.endswith("_ms")]:
    out[key[:-3] + "_best_ms"] = min(out[key])
for ctx, _ in ctxs.values():
    ctx.close()
print(json.dumps(out), flush=True)
