"""Light-direction shadows under a first-hit isosurface on the C2 shape (256^3 bonsai stand-in, 1080p, dt 0.5, f16 out, lit, R = 4): ms per
frame, one frame per launch and 128 orbit frames per launch, interleaved, best of three groups per repetition, at iso 0.1 (just above
the stand-in's air) and iso 0.4 (inside the canopy), for
  iso_{air,canopy}_{l45,graze}_off   shadows off: the isosurface kernels every render without shadows launches
  iso_{air,canopy}_{l45,graze}_on    shadows on (strength 0.7, bias 2): the shadow kernels
under a light at 45 degrees to the view axis (l45) and a grazing one, 85 degrees from it (graze): the more a light grazes, the more of
the visible surface faces away from it or lies behind other material, and the longer the unshadowed rays travel to the box's exit.
Per configuration: the empty fraction, S_ref, S_sampled (the primary ray's: shadow iterations count in neither, so the on and off rows
must agree), the frame and step checksums, the share of the frame's pixels that hit, and for the on rows the share of the hits that is
shadowed -- counted on a second frame with ambient 0, specular 0, diffuse 1 and strength 1, where a shadowed pixel is exactly 0.
The cost to explain is each on row against the off row beside it.
usage: tools/shadow_quick.py [--reps N]"""
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
SHADOWS = (0.7, 2.0)
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


def empty_fraction(ctx):
    f = C.c_double()
    N.check(ctx.handle, N.lib().vk_volume_empty_fraction(ctx.handle, C.byref(f)))
    return f.value


cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
orbit = [V.Camera(1.0, 0.5, 1.0 + 6.28318 * j / 1024, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix() for j in range(B)]
# the view axis (from the target to the eye) and a unit vector across it: a light `deg` degrees from the view axis
view = np.frombuffer(cam.get_proj_view_matrix(), np.float32)[:3].astype(np.float64) - 0.5
view /= np.linalg.norm(view)
across = np.cross(view, (0.0, 1.0, 0.0))
across /= np.linalg.norm(across)


def light(deg):
    d = np.cos(np.radians(deg)) * view + np.sin(np.radians(deg)) * across
    return dict(direction=tuple(float(v) for v in d), ambient=0.2, diffuse=0.8, specular=0.4, shininess=24.0)


configs = []  # name, threshold, light, shadows
for label, iso in (("air", AIR), ("canopy", CANOPY)):
    for lname, deg in (("l45", 45.0), ("graze", 85.0)):
        for on in (False, True):
            configs.append(("iso_%s_%s_%s" % (label, lname, "on" if on else "off"), iso, light(deg), SHADOWS if on else None))
ctxs = {}
out = {"lib": os.environ.get("VK_LIB", "product")}
for name, iso, li, sh in configs:
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA16F)
    ctx.set_isosurface(iso, (0.9, 0.7, 0.4), 4)
    ctx.set_lighting(**li)
    if sh is not None:
        ctx.set_shadows(*sh)
    V.VolumeTexture.generate_standin(ctx, (256,) * 3)
    ctx.update()
    ctx.reset_step_counts()
    V.RaycastPipeline(dt_scale=DT, flags=V.RENDER_COUNT).record(ctx)
    frame = ctx.read_backbuffer()
    out[name + "_crc"] = "%08x" % zlib.crc32(frame.tobytes())  # the frame, for A/B runs: both sides must agree
    out[name + "_steps_crc"] = "%08x" % zlib.crc32(ctx.read_steps().tobytes())
    s_ref, s_sampled = ctx.step_counts()
    out[name + "_empty_fraction"] = round(empty_fraction(ctx), 4)
    out[name + "_s_ref"], out[name + "_s_sampled"] = int(s_ref), int(s_sampled)
    hit = (frame[..., :3] > 0).any(axis=2)  # (ambient 0.2 on a positive colour: a pixel that hit is not black)
    out[name + "_hit_share"] = round(float(hit.mean()), 4)
    if sh is not None:  # the shadow mask: nothing but the diffuse term, a shadowed point loses all of it
        ctx.set_isosurface(iso, (1.0, 1.0, 1.0), 4)
        ctx.set_lighting(**dict(li, ambient=0.0, diffuse=1.0, specular=0.0))
        ctx.set_shadows(1.0, sh[1])
        V.RaycastPipeline(dt_scale=DT).record(ctx)
        black = (ctx.read_backbuffer()[..., :3] == 0).all(axis=2)
        out[name + "_shadowed_share_of_hits"] = round(float((black & hit).sum()) / max(1, int(hit.sum())), 4)
        ctx.set_isosurface(iso, (0.9, 0.7, 0.4), 4)
        ctx.set_lighting(**li)
        ctx.set_shadows(*sh)
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
for name, _, _, sh in configs:
    if sh is not None:
        off = name[:-2] + "off"
        assert (out[name + "_s_ref"], out[name + "_s_sampled"], out[name + "_steps_crc"]) == (out[off + "_s_ref"], out[off + "_s_sampled"], out[off + "_steps_crc"])
        for k in ("single_ms", "orbit128_ms_per_frame"):
            out[name + "_over_off_" + k] = round(min(out[name + "_" + k]) / min(out[off + "_" + k]), 3)
for ctx in ctxs.values():
    ctx.close()
print(json.dumps(out), flush=True)
