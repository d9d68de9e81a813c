"""The resample pass (vk_volume_resample) beside its yardsticks.  Cases, on LINEAR and PACKED each:
  area_1024_to_512     a 1024^3 u8 site-percolation field (density 79 / 256) to 512^3, VK_RESAMPLE_AREA (every source voxel read once)
  linear_z2            512 x 512 x 300 u16 to 512 x 512 x 600, VK_RESAMPLE_LINEAR (the anisotropic scan made isotropic)
  crop_512             the 512^3 centre of the 1024^3 field, VK_RESAMPLE_NEAREST (a copy)
  window_u16_to_u8     1024^3 u16 to u8 under the window 0.1 .. 0.6 at the same size, VK_RESAMPLE_NEAREST with the value map
Per case and layout:
  kernel_ms    the kernel alone between the context's timer events (vk_debug_set_param "resample_timing" 1), best of --reps calls;
               AREA: passes_kernel_ms the three axis passes through f32 intermediates ("resample_area_passes" 1), the structure not chosen
  call_ms      the blocking call end to end on the host with dense_out (it includes the copy of the result to host memory)
  install_ms   one installing call (the kernel and the re-layout of the result), run last
  src_bytes, out_bytes, src_stream_ms, out_stream_ms, out_write_ms
               the yardsticks: a sum over an array of the source layout's bytes and of the output's bytes with 16-byte loads
               (tools/ubench/stream_read.hip, as tools/filter_quick.py runs it), and a fill of the output's bytes (torch's fill_ between
               two events): a streaming write
and for the 512-sized case linear_z2 scipy.ndimage.zoom(order=1, mode="nearest", grid_mode=True) on one CPU thread (cpu_ms).
usage: tools/resample_quick.py [--reps N] [--small]   (--small: 256^3 and 128-sized stand-ins of every case, seconds)"""
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import numpy as np
import torch

import vokselis_amd as V

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
small = "--small" in sys.argv
N = 256 if small else 1024


def cell_bytes(dims, cell):
    n = 64
    for d in dims:
        n *= ((d - 1) >> 2) + 2
    return n * cell


def stream_ms(sizes):
    src, exe = os.path.join(HERE, "ubench", "stream_read.hip"), os.path.join(HERE, "ubench", "_build", "stream_read")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    r = subprocess.run([exe] + [str(n) for n in sizes], capture_output=True, text=True, check=True, timeout=300)
    return {int(k): v for k, v in json.loads(r.stdout).items()}


def write_ms(nbytes):
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    best = 1e9
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        buf.fill_(7)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    del buf
    return best


def percolation(n):
    rng = np.random.default_rng(31)
    vol = np.empty((n, n, n), np.uint8)
    for z in range(n):  # a plane at a time: no float64 copy of the whole field
        vol[z] = np.where(rng.integers(0, 256, (n, n), dtype=np.uint8) < 79, 255, 0)
    return vol


def cases():
    field = percolation(N)
    h, q = N // 2, N // 4
    yield "area_1024_to_512", field, "u8", dict(dims=(h, h, h), mode="area")
    yield "crop_512", field, "u8", dict(box=((q, q, q), (q + h, q + h, q + h)), mode="nearest")
    wide = field.astype(np.uint16) * np.uint16(257)
    del field
    yield "window_u16_to_u8", wide, "u16", dict(mode="nearest", fmt="u8", window=(0.1, 0.6))
    del wide
    rng = np.random.default_rng(32)
    scan = rng.integers(0, 65536, (300 * N // 1024, N // 2, N // 2), dtype=np.uint16)
    yield "linear_z2", scan, "u16", dict(dims=(N // 2, N // 2, 2 * scan.shape[0]), mode="linear")


out = {}
names = []
for cname, vol, kind, kw in cases():
    dims = tuple(reversed(vol.shape))
    for layout, lname in ((V.LAYOUT_LINEAR, "linear"), (V.LAYOUT_PACKED, "packed")):
        name = f"{cname}_{lname}"
        names.append(name)
        print(name, file=sys.stderr, flush=True)
        esz = 1 if kind == "u8" else 2
        out[name + "_src_bytes"] = vol.size * esz if layout == V.LAYOUT_LINEAR else cell_bytes(dims, 8 if kind == "u8" else 16)
        ctx = V.Context(64, 64, backbuffer=(64, 64), out_format=V.OUT_RGBA16F)
        try:
            V.VolumeTexture(ctx, vol, layout=layout, **(dict(fmt=V.FMT_R16_UNORM) if kind == "u16" else {}))
            ctx.set_param("resample_timing", 1)
            best_k, best_c = 1e9, 1e9
            for _ in range(reps):
                t0 = time.perf_counter()
                got, res = ctx.resample_volume(install=False, out=True, **kw)
                best_c = min(best_c, (time.perf_counter() - t0) * 1e3)
                best_k = min(best_k, ctx.timer_elapsed_ms())
            out[name + "_out_dims"] = list(res.dims)
            out[name + "_out_bytes"] = int(got.nbytes)
            if "box" in kw:  # the crop reads its box only
                out[name + "_src_bytes"] = out[name + "_src_bytes"] // 8
            out[name + "_kernel_ms"], out[name + "_call_ms"] = round(best_k, 4), round(best_c, 3)
            if kw["mode"] == "area":  # the other structure: three axis passes through f32 intermediates
                ctx.set_param("resample_area_passes", 1)
                best_k = 1e9
                for _ in range(reps):
                    again, _ = ctx.resample_volume(install=False, out=True, **kw)
                    best_k = min(best_k, ctx.timer_elapsed_ms())
                out[name + "_passes_kernel_ms"] = round(best_k, 4)
                out[name + "_passes_same_bits"] = bool((again == got).all())
                ctx.set_param("resample_area_passes", 0)
                ctx.set_param("resample_area_unroll", 0)  # ... and the fused kernel with the table-driven loops
                best_k = 1e9
                for _ in range(reps):
                    again, _ = ctx.resample_volume(install=False, out=True, **kw)
                    best_k = min(best_k, ctx.timer_elapsed_ms())
                out[name + "_loops_kernel_ms"] = round(best_k, 4)
                out[name + "_loops_same_bits"] = bool((again == got).all())
                ctx.set_param("resample_area_unroll", 1)
                del again
            ctx.set_param("resample_timing", 0)
            t0 = time.perf_counter()
            ctx.resample_volume(install=True, **kw)
            ctx.sync()
            out[name + "_install_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            if cname == "linear_z2" and layout == V.LAYOUT_LINEAR:
                try:
                    from scipy import ndimage

                    t0 = time.perf_counter()
                    ref = ndimage.zoom(vol.astype(np.float32), (2.0, 1.0, 1.0), order=1, mode="nearest", grid_mode=True)
                    out[cname + "_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                    out[cname + "_cpu_max_diff_lsb"] = float(np.abs(ref - got.astype(np.float32)).max())
                    del ref
                except ImportError:
                    out[cname + "_cpu_ms"] = None
            del got
        finally:
            ctx.close()
    del vol
sizes = sorted({out[n + "_src_bytes"] for n in names} | {out[n + "_out_bytes"] for n in names})
for rep in range(reps):
    ms = stream_ms(sizes)
    for n in names:
        out[n + "_src_stream_ms"] = min(out.get(n + "_src_stream_ms", 1e9), ms[out[n + "_src_bytes"]])
        out[n + "_out_stream_ms"] = min(out.get(n + "_out_stream_ms", 1e9), ms[out[n + "_out_bytes"]])
for n in names:
    out[n + "_out_write_ms"] = round(write_ms(out[n + "_out_bytes"]), 4)
print(json.dumps(out), flush=True)
