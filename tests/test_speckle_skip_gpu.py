"""Lone-speckle cells on the MI355X (vk_tf.hpp: speckle_code / speckle_proven; march() in vk_march.hpp): a distance byte >= 128 lets a lane
prove a sample transparent from the weights it already has, and step on without fetching the cell.  An exact optimisation: frames,
per-pixel step counts, S_ref and S_sampled are those of a march that samples every such step.

The volume: 40 x 36 x 44 u8, air 0..20 with lone voxels of 26, 27, 41 and 255 (some on faces, on edges and in a corner of the volume), one
6^3 dense blob and two adjacent hot voxels.  The air is a checkerboard of 10..20 and 0..20, so that every cell holds a cold tap >= 10:
next to a 255 voxel the limit is then floor(16 * 15 / 245) = 0 and the cell carries no code, which the all-255 variant relies on.
96 x 64 frames at dt_scale 0.5 and 1.0 from three cameras (outside, grazing a face, eye inside), PACKED and PACKED_PAIRS.
Single-frame launches take the probe-ahead kernel by default, which reads the codes as cells to sample; the kernel that decodes them is
the batches' (debug parameter probe_ahead = 0 gives it to a single frame, 1 the probe-ahead kernel)."""
import numpy as np
import pytest

from gpu_helpers import V, _synced  # noqa: F401
from tf_helpers import band_pass_table

pytestmark = pytest.mark.gpu

NX, NY, NZ = 40, 36, 44
W, H = 96, 64
CAMS = {"outside": (1.1, 0.45, 0.9, (0.5, 0.5, 0.5), W / H),
        "grazing": (1.2, 0.03, 2.1, (0.5, 0.02, 0.5), W / H),
        "inside": (0.2, -0.3, 4.0, (0.45, 0.55, 0.4), W / H)}
DTS = (0.5, 1.0)
LAYOUTS = ("PACKED", "PACKED_PAIRS")


def _volume(hot_all_255=False):
    rng = np.random.default_rng(20260)
    z, y, x = np.meshgrid(np.arange(NZ), np.arange(NY), np.arange(NX), indexing="ij")
    vol = np.where(((x + y + z) & 1) == 0, rng.integers(10, 21, (NZ, NY, NX)), rng.integers(0, 21, (NZ, NY, NX))).astype(np.uint8)
    hot = []  # (z, y, x, value): lone voxels, no two within one cell of each other
    taken = np.zeros((NZ, NY, NX), bool)
    taken[18:26, 10:18, 20:28] = True  # around the blob
    taken[32:37, 6:11, 28:34] = True   # around the adjacent pair
    fixed = [(0, 0, 0), (NZ - 1, NY - 1, NX - 1), (0, NY - 1, 17), (21, 0, 0), (NZ - 1, 9, 0),              # corners and edges
             (0, 17, 23), (30, 0, 11), (12, 20, 0), (NZ - 1, 5, 30), (9, NY - 1, 8), (33, 25, NX - 1)]      # faces
    draws = [tuple(int(v) for v in p) for p in zip(rng.integers(0, NZ, 400), rng.integers(0, NY, 400), rng.integers(0, NX, 400))]
    for k, (pz, py, px) in enumerate(fixed + draws):
        lo = (max(pz - 2, 0), max(py - 2, 0), max(px - 2, 0))
        if taken[lo[0]:pz + 3, lo[1]:py + 3, lo[2]:px + 3].any():
            continue
        taken[pz, py, px] = True
        hot.append((pz, py, px, (26, 27, 41, 255)[k % 4]))
    for pz, py, px, v in hot:
        vol[pz, py, px] = 255 if hot_all_255 else v
    vol[19:25, 11:17, 21:27] = rng.integers(120, 201, (6, 6, 6))  # the dense blob
    vol[34, 8, 30] = 255 if hot_all_255 else 30                     # two adjacent hot voxels
    vol[34, 8, 31] = 255 if hot_all_255 else 35
    assert len(hot) >= 60 and {v for *_, v in hot} == {26, 27, 41, 255}
    return vol


@pytest.fixture(scope="module")
def vol():
    return _volume()


@pytest.fixture(scope="module")
def oracle_refs(O, vol):
    """(camera, dt) -> (camera blob, the oracle's per-pixel steps, its sums of steps and of steps in non-empty cells): computed once."""
    out = {}
    for cname, cam in CAMS.items():
        blob = O.camera_blob(*cam)
        for dt in DTS:
            _, steps, sampled = O.render(blob, vol, W, H, dt_scale=dt)
            out[cname, dt] = (blob, steps, int(steps.sum(dtype=np.uint64)), int(sampled.sum(dtype=np.uint64)))
    return out


def _render(V, ctx, blob, dt, flags):
    """(frame, steps, (S_ref, S_sampled), speckle census) of one counted render."""
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
    ctx.set_camera_blob(blob)
    ctx.reset_step_counts()
    V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=dt, flags=flags | V.RENDER_COUNT).record(ctx)
    return ctx.read_backbuffer().copy(), ctx.read_steps().copy(), tuple(int(v) for v in ctx.step_counts()), ctx.speckle_census()


def _same(a, b):
    return bool((a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1] == b[1]).all())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("cname", list(CAMS))
def test_proven_steps_change_no_bit(V, vol, oracle_refs, layout, dt, cname):
    blob, ref_steps, s_ref, s_sampled = oracle_refs[cname, dt]
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout))
        ctx.set_param("probe_ahead", 0)  # the kernel that decodes
        probe = _render(V, ctx, blob, dt, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS)
        others = {name: _render(V, ctx, blob, dt, fl) for name, fl in (("default", 0), ("no skip", V.RENDER_NO_SKIP), ("force", V.RENDER_FORCE_SKIP),
                                                                         ("safe", V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS | V.RENDER_SAFE))}
        V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
        V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=dt, flags=V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS).record(ctx)
        prod = ctx.read_backbuffer().copy()
        ctx.set_param("probe_ahead", 1)  # the probe-ahead kernel: the codes are cells to sample
        others["probe ahead"] = _render(V, ctx, blob, dt, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS)
    finally:
        ctx.close()
    print(f"\n{layout} dt {dt} {cname}: S_ref {probe[2][0]} S_sampled {probe[2][1]} (oracle {s_ref} / {s_sampled}); census {probe[3]}; "
          f"no-skip census {others['no skip'][3]}")
    for name, other in others.items():
        assert _same(other, probe), f"policy '{name}': frame or per-pixel steps differ from probe-every-trip"
    assert (prod.view(np.uint32) == probe[0].view(np.uint32)).all(), "the production kernel differs from the COUNT kernel"
    assert (probe[1] == ref_steps).all()
    assert probe[2] == (s_ref, s_sampled)
    assert others["no skip"][2][0] == s_ref
    assert probe[3]["lane_proven_steps"] > 0
    assert others["no skip"][3]["lane_proven_steps"] == 0 and others["probe ahead"][3]["lane_proven_steps"] == 0
    assert others["probe ahead"][2] == probe[2]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_255_voxel_is_never_proven(V, layout, O):
    vol255 = _volume(hot_all_255=True)
    blob = O.camera_blob(*CAMS["outside"])
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, vol255, layout=getattr(V, "LAYOUT_" + layout))
        ctx.set_param("probe_ahead", 0)
        got = _render(V, ctx, blob, 0.5, V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS)
        plain = _render(V, ctx, blob, 0.5, V.RENDER_NO_SKIP)
    finally:
        ctx.close()
    assert got[3]["lane_proven_steps"] == 0
    assert got[3]["wave_zero_alpha_execs"] > 0  # (the speckle cells are still there, and sampled)
    assert _same(got, plain)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_single_frame_probe_ahead_equals_the_batch(V, vol, O, layout):
    import torch

    w, h = 200, 120
    cams = [O.camera_blob(1.0 + 0.1 * k, 0.4 - 0.2 * k, 0.7 + 0.9 * k, (0.5, 0.5, 0.5), w / h) for k in range(3)]
    ctx = V.Context(w, h, backbuffer=(w, h), out_format=V.OUT_RGBA32F)
    try:
        ctx.set_param("probe_ahead", 1)  # the probe-ahead kernel for the single frames whatever else is in flight
        V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout))
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5, flags=V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS)
        singles = []
        for c in cams:
            ctx.set_camera_blob(c)
            pipe.record(ctx)
            singles.append(ctx.read_backbuffer().copy())
        ctx.set_param("probe_ahead", 2)  # the default: batches march with the leaner kernel
        frames = _synced(torch.zeros((3, h, w, 4), dtype=torch.float32, device="cuda"))
        V.render_batch(ctx, pipe, cams, frames.data_ptr(), tile_size=32)
        ctx.sync()
        got = frames.cpu().numpy()
        ctx.set_camera_blob(cams[0])
        plain = _render(V, ctx, cams[0], 0.5, V.RENDER_NO_SKIP)
    finally:
        ctx.close()
    for k in range(3):
        assert (got[k].view(np.uint32) == singles[k].view(np.uint32)).all(), ("batch frame", k)
    assert (plain[0].view(np.uint32) == singles[0].view(np.uint32)).all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_table_set_and_cleared_restores_the_codes(V, vol, O, layout):
    blob = O.camera_blob(*CAMS["outside"])
    fl = V.RENDER_FORCE_SKIP | V.RENDER_PROBE_ALWAYS
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + layout))
        ctx.set_param("probe_ahead", 0)
        first = _render(V, ctx, blob, 0.5, fl)
        ctx.set_transfer_function(band_pass_table())
        under = _render(V, ctx, blob, 0.5, fl)
        under_plain = _render(V, ctx, blob, 0.5, V.RENDER_NO_SKIP)
        ctx.set_transfer_function(None)
        third = _render(V, ctx, blob, 0.5, fl)
    finally:
        ctx.close()
    assert _same(under, under_plain) and under[3]["lane_proven_steps"] == 0  # maps under a table carry no codes
    assert _same(first, third)
    assert first[2] == third[2] and first[3] == third[3] and first[3]["lane_proven_steps"] > 0
