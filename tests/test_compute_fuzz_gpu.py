"""The compute twin (VK_MODE_COMPUTE_NEAREST) on the MI355X over the shared fuzz cases (tests/compute_cases.py), against the C oracle, which
the CPU suite holds to an independent float64 reference (tests/test_compute_fuzz_cpu.py).

For every case, on LINEAR (the literal twin: the two dense volumes), PACKED (the records kernel) and AUTO:
- per-pixel step counts equal the oracle's, under every policy below;
- the literal twin's colour is within TOL of the oracle's, with NaN exactly where the oracle has NaN (and the same infinities);
- the records kernel gives the same bits under the default policy, RENDER_NO_SKIP, each request ring (set_param("pair_ring", 4 / 6 / 42))
  and pair_walk_min 2 and 64, and AUTO gives PACKED's frame;
- the records kernel gives the literal twin's frame bit for bit, but on the cases tagged `divergent` (vk_compute.hpp: the short form of
  the shade), and there, its colour is held to nothing but the other records frames;
- the production kernel (no RENDER_COUNT) gives the COUNT kernel's frame bit for bit;
- RGBA16F output is the round-to-nearest-even of the RGBA32F frame (the cases marked `half`);
- pixels outside a tile keep the clear colour;
- on PACKED, a 3-frame render_batch gives the three single launches bit for bit (the cases without a tile).
The walk cases run down 128..256-voxel axes; four of them put the eye 45, 150 and 300 units away at the smallest dt the library accepts,
where every t = t + dt rounds up (two against a single slab): there the WALK's hops must allow for that drift to keep SKIP == NO_SKIP.
NaN compares equal to NaN in the bitwise checks (its payload is not part of the contract).  A slice of C3 (VK_MODE_PROCEDURAL, no volume)
draws cameras, dt and tiles the same way, with Uniform.time up to 1e5: steps, colour within TOL and RGBA16F as RNE against the oracle.
Every mismatch is collected and reported together with the case that shows it."""
import time

import numpy as np
import pytest

import compute_cases
from gpu_helpers import TOL, V, _synced  # noqa: F401
from test_compute_fuzz_cpu import colour_mismatch

pytestmark = pytest.mark.gpu

RECORD_VARIANTS = (("no skip", (), "NO_SKIP"), ("ring 4", (("pair_ring", 4),), ""), ("ring 6", (("pair_ring", 6),), ""),
                   ("ring 42", (("pair_ring", 42),), ""), ("walk_min 2", (("pair_walk_min", 2),), ""),
                   ("walk_min 64", (("pair_walk_min", 64),), ""))
DEFAULTS = (("pair_ring", 0), ("pair_walk_min", 4))


def _context(V, c, layout, out):
    ctx = V.Context(c.W, c.H, backbuffer=(c.W, c.H), out_format=out)
    try:
        V.VolumeTexture(ctx, c.den, c.nrm, layout=getattr(V, "LAYOUT_" + layout))
    except BaseException:
        ctx.close()
        raise
    return ctx


def _render(V, ctx, cam, dt, tile, flags, mode=None):
    """(frame, steps); steps only under RENDER_COUNT."""
    from vokselis_amd import _native as N

    N.check(ctx.handle, N.lib().vk_backbuffer_clear(ctx.handle))
    ctx.set_camera_blob(cam)
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_COMPUTE_NEAREST if mode is None else mode, dt_scale=dt, flags=flags).record(ctx, tile)
    return ctx.read_backbuffer().copy(), (ctx.read_steps().copy() if flags & V.RENDER_COUNT else None)


def _same(a, b):
    """Bitwise equal, NaN equal to NaN."""
    a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a32.view(np.uint32) == b32.view(np.uint32)) | (np.isnan(a32) & np.isnan(b32))


def _rne16(frame):
    return np.asarray(frame, np.float32).astype(np.float16)


def _same16(h, want):
    return (h.view(np.uint16) == want.view(np.uint16)) | (np.isnan(h) & np.isnan(want))


def _tile_mask(W, H, tile):
    m = np.zeros((H, W), bool)
    if tile is None:
        m[:] = True
    else:
        tx, ty, tw, th = tile
        m[max(ty, 0):max(min(ty + th, H), 0), max(tx, 0):max(min(tx + tw, W), 0)] = True
    return m


def test_compute_fuzz_against_the_oracle(V, O):
    import torch

    start = time.perf_counter()
    fails, worst = [], {"LINEAR": (0.0, None), "PACKED": (0.0, None)}
    renders = halves = batches = 0

    def fail(what, msg):
        fails.append((what, msg))

    for c in compute_cases.cases(O):
        cam = O.camera_blob(*c.cam)
        ref, ref_steps, _ = O.render(cam, c.den, c.W, c.H, mode=O.MODE_COMPUTE_NEAREST, volume2=c.nrm, dt_scale=c.dt, tile=c.tile)
        m = _tile_mask(c.W, c.H, c.tile)
        frames = {}
        for lay in ("LINEAR", "PACKED", "AUTO"):
            what = (c, lay)
            ctx = _context(V, c, lay, V.OUT_RGBA32F)
            try:
                got = [("default", *_render(V, ctx, cam, c.dt, c.tile, V.RENDER_COUNT))]
                if lay == "PACKED":
                    for name, params, flag in RECORD_VARIANTS:
                        for k, v in params:
                            ctx.set_param(k, v)
                        got.append((name, *_render(V, ctx, cam, c.dt, c.tile, V.RENDER_COUNT | (V.RENDER_NO_SKIP if flag else 0))))
                        for k, v in DEFAULTS:
                            ctx.set_param(k, v)
                prod, _ = _render(V, ctx, cam, c.dt, c.tile, 0)
            finally:
                ctx.close()
            renders += len(got) + 1
            img, steps = got[0][1], got[0][2]
            frames[lay] = img
            for name, _, osteps in got:
                if not (osteps[m] == ref_steps[m]).all():
                    fail(what, f"'{name}': steps differ from the oracle at {int((osteps[m] != ref_steps[m]).sum())} pixels")
            for name, other, _ in got[1:]:
                if not _same(other, img).all():
                    fail(what, f"'{name}' differs from the default policy at {int((~_same(other, img)).any(axis=2).sum())} pixels")
            if not _same(prod, img).all():
                fail(what, "the production kernel differs from the COUNT kernel")
            if c.tile is not None and not (img[~m] == [0.0, 0.0, 0.0, 1.0]).all():
                fail(what, "pixels outside the tile were written")
            if lay == "LINEAR" or (lay == "PACKED" and not c.divergent):
                err, odd = colour_mismatch(img[m][..., :3], ref[m][..., :3], TOL)
                if not (err <= TOL and odd == 0):
                    fail(what, f"colour error {err:.3g} > {TOL} or {odd} pixels whose NaN / infinities differ from the oracle's")
                if err > worst[lay][0] or worst[lay][1] is None:
                    worst[lay] = (err, c.name)
            if c.half:
                ctx = _context(V, c, lay, V.OUT_RGBA16F)
                try:
                    h, _ = _render(V, ctx, cam, c.dt, c.tile, 0)
                finally:
                    ctx.close()
                halves += 1
                renders += 1
                if not _same16(h, _rne16(prod)).all():
                    fail(what, "RGBA16F output is not the RNE of the RGBA32F frame")
        if not c.divergent and not _same(frames["PACKED"], frames["LINEAR"]).all():
            fail((c, "PACKED"), f"differs from LINEAR at {int((~_same(frames['PACKED'], frames['LINEAR'])).any(axis=2).sum())} pixels")
        if not _same(frames["AUTO"], frames["PACKED"]).all():
            fail((c, "AUTO"), "differs from PACKED")
        if c.tile is None:  # three frames in one launch against the three single launches
            cams = [cam] + [O.camera_blob(c.cam[0], c.cam[1], c.cam[2] + 0.3 * k, c.cam[3], c.cam[4]) for k in (1, 2)]
            ctx = _context(V, c, "PACKED", V.OUT_RGBA32F)
            try:
                pipe = V.RaycastPipeline(V.MODE_COMPUTE_NEAREST, dt_scale=c.dt)
                singles = [_render(V, ctx, b, c.dt, None, 0)[0] for b in cams]
                out = _synced(torch.zeros((3, c.H, c.W, 4), dtype=torch.float32, device="cuda"))
                V.render_batch(ctx, pipe, cams, out.data_ptr(), tile_size=32)
                ctx.sync()
                out = out.cpu().numpy()
            finally:
                ctx.close()
            batches += 1
            renders += 4
            if not _same(singles[0], frames["PACKED"]).all():
                fail((c, "batch"), "the single launch differs from the default policy's frame")
            for k in range(3):
                if not _same(out[k], singles[k]).all():
                    fail((c, "batch"), f"frame {k} of the batch differs from its single launch")
    elapsed = time.perf_counter() - start
    print(f"\ncompute fuzz: {compute_cases.N_CASES} cases, {renders} renders ({halves} RGBA16F, {batches} batches), {elapsed:.1f} s; "
          "largest colour error vs the oracle: " + ", ".join(f"{lay} {e:.3g} ({name})" for lay, (e, name) in worst.items()))
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    assert halves >= 18 and batches >= 30
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"


def test_procedural_slice_against_the_oracle(V, O):
    """C3 at the drawn cameras, dt and tiles, Uniform.time up to 1e5."""
    fails, worst = [], 0.0
    for name, args, kind, W, H, dt, tile, t, half in compute_cases.procedural_cases():
        cam = O.camera_blob(*args)
        ref, ref_steps = O.render_procedural(cam, W, H, dt_scale=dt, time=t, tile=tile)
        m = _tile_mask(W, H, tile)
        for out in (V.OUT_RGBA32F,) + ((V.OUT_RGBA16F,) if half else ()):
            ctx = V.Context(W, H, backbuffer=(W, H), out_format=out)
            try:
                ctx.global_uniform.time = t
                V.native.check(ctx.handle, V.native.lib().vk_set_uniform(ctx.handle, ctx.global_uniform.to_bytes()))
                img, steps = _render(V, ctx, cam, dt, tile, V.RENDER_COUNT, mode=V.MODE_PROCEDURAL)
            finally:
                ctx.close()
            what = (name, args, W, H, dt, tile, t, "RGBA16F" if out == V.OUT_RGBA16F else "RGBA32F")
            if not (steps[m] == ref_steps[m]).all():
                fails.append((what, f"steps differ from the oracle at {int((steps[m] != ref_steps[m]).sum())} pixels"))
            if out == V.OUT_RGBA32F:
                f32 = img
                err, odd = colour_mismatch(img[m][..., :3], ref[m][..., :3], TOL)
                worst = max(worst, err)
                if not (err <= TOL and odd == 0):
                    fails.append((what, f"colour error {err:.3g}"))
                if ref_steps[m].max(initial=0) == 0 and tile is None:
                    fails.append((what, "the case marches nothing"))
            elif not _same16(img, _rne16(f32)).all():
                fails.append((what, "RGBA16F output is not the RNE of the RGBA32F frame"))
    print(f"\nC3 slice: {len(compute_cases.procedural_cases())} cases, largest colour error {worst:.3g}")
    for what, msg in fails[:20]:
        print("FAIL", what, msg)
    assert not fails, f"{len(fails)} mismatches; first: {fails[0]}"
