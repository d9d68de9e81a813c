"""vk_volume_histogram on the MI355X through its entry point: the two exact anchors on all their layouts, the
grid-stride loop and the merges under hist_max_blocks and hist_flush_passes, the collapsed and the contended counting paths on a constant
and a uniform random volume, NULL outputs, VK_HIST_CLIP_BOX against the explicit box, the state the pass must leave alone, a call inside a
frame, device memory over repeated calls, every refusal with its status, and the Python Histogram's mean / std / window.  The kernels are
held to the restatement over the shared cases in tests/test_hist_fuzz_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import hist_helpers as HH
import np_hist_reference as NH
import test_hist_fuzz_cpu as AN  # the anchors' volumes
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
SEVEN = (("u8", "LINEAR"), ("u8", "PACKED"), ("u8", "PACKED_PAIRS"), ("f16", "LINEAR"), ("f16", "PACKED"), ("u16", "LINEAR"), ("u16", "PACKED"))


def _ctx(V, vol, kind=None, layout="PACKED", size=(32, 24)):
    ctx = V.Context(size[0], size[1], backbuffer=size, out_format=V.OUT_RGBA32F)
    try:
        if vol is not None:
            kind = kind or {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}[vol.dtype]
            HH.upload(V, ctx, vol, kind, layout)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _code(V, fn):
    with pytest.raises(V.VokselisError) as e:
        fn()
    return e.value.code, str(e.value)


def _same(a, b, sums=False):
    d = HH.integer_part_differences(HH.from_histogram(a), HH.from_histogram(b))
    if sums and (a.stats.sum != b.stats.sum or a.stats.sum_sq != b.stats.sum_sq):
        d.append("sums differ")
    return d


@pytest.fixture(scope="module")
def volumes():
    rng = np.random.default_rng(11)
    v = {"odd": rng.integers(0, 256, (7, 20, 33)).astype(np.uint8),           # 33 x 20 x 7
         "passes": rng.integers(0, 65536, (40, 64, 64)).astype(np.uint16),    # 64 x 64 x 40: 163 840 voxels, more than one pass for one block
         "constant": np.full((64, 64, 64), 93, np.uint8),
         "uniform": rng.integers(0, 256, (64, 64, 64)).astype(np.uint8),
         "f16": rng.normal(0.4, 0.3, (12, 20, 28)).astype(np.float16)}
    for a in v.values():
        a.setflags(write=False)
    return v


@pytest.mark.parametrize("kind, layout", [s for s in SEVEN if s[0] != "f16"])
def test_exact_anchors_on_every_layout(V, kind, layout):  # noqa: F811
    """bins = 256 over [0, 1]: an R8 volume's counts are bincount(v), an R16_UNORM volume's bincount(v >> 8) -- over every value of the format."""
    vol = AN.all_values(kind)
    shift = 0 if kind == "u8" else 8
    ctx = _ctx(V, vol, kind, layout)
    try:
        h = ctx.volume_histogram(256, (0.0, 1.0))
        assert (h.counts == np.bincount(vol.ravel().astype(np.int64) >> shift, minlength=256).astype(np.uint64)).all()
        assert (h.n_voxels, h.n_nan, h.n_below, h.n_above, h.n_finite) == (vol.size, 0, 0, 0, vol.size)
        assert h.stats.min == 0.0 and h.stats.max == float(np.iinfo(vol.dtype).max) and h.min == 0.0 and h.max == 1.0
        box = ((1, 2, 1), (8, 7, 4)) if kind == "u8" else ((3, 5, 2), (64, 61, 15))
        sub = vol[box[0][2]:box[1][2], box[0][1]:box[1][1], box[0][0]:box[1][0]]
        h = ctx.volume_histogram(256, (0.0, 1.0), box)
        assert (h.counts == np.bincount(sub.ravel().astype(np.int64) >> shift, minlength=256).astype(np.uint64)).all() and h.n_voxels == sub.size
        assert h.stats.sum == float(sub.astype(np.int64).sum()) and h.stats.sum_sq == float((sub.astype(np.int64) ** 2).sum())
    finally:
        ctx.close()


@pytest.mark.parametrize("name, layouts", [("odd", ("LINEAR", "PACKED", "PACKED_PAIRS")), ("passes", ("LINEAR", "PACKED"))])
def test_capped_grids_and_early_merges_give_the_uncapped_result(V, volumes, name, layouts):  # noqa: F811
    vol = volumes[name]
    nz, ny, nx = vol.shape
    box = ((1, 0, 1), (nx, ny - 1, nz))
    for layout in layouts:
        ctx = _ctx(V, vol, None, layout)
        try:
            for b in (None, box):
                free = ctx.volume_histogram(1000, (0.0, 1.0), b)
                assert free.n_voxels == (vol.size if b is None else (nx - 1) * (ny - 1) * (nz - 1)) and int(free.counts.sum()) == free.n_voxels
                for blocks in (1, 2, 3):
                    for flush in (0, 1, 3):
                        ctx.set_param("hist_max_blocks", blocks)
                        ctx.set_param("hist_flush_passes", flush)
                        capped = ctx.volume_histogram(1000, (0.0, 1.0), b)
                        assert not _same(capped, free, sums=True), (layout, b, blocks, flush, _same(capped, free, sums=True))  # (integer formats: the sums are exact in any order)
                ctx.set_param("hist_max_blocks", 0)
                ctx.set_param("hist_flush_passes", 0)
                assert not _same(ctx.volume_histogram(1000, (0.0, 1.0), b), free, sums=True)
        finally:
            ctx.close()


@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_constant_and_uniform_volumes_give_their_exact_counts(V, volumes, layout):  # noqa: F811
    """The collapsed path (a whole wave in one slot) and the contended one (every voxel another bin)."""
    for name in ("constant", "uniform"):
        vol = volumes[name]
        ctx = _ctx(V, vol, "u8", layout)
        try:
            for bins, shift in ((256, 0), (4096, None), (1, 8)):
                h = ctx.volume_histogram(bins, (0.0, 1.0))
                if shift is not None:
                    want = np.bincount(vol.ravel().astype(np.int64) >> shift, minlength=bins).astype(np.uint64)
                else:
                    want = NH.histogram(vol, "u8", bins, (0.0, 1.0))["counts"]
                assert (h.counts == want).all() and int(h.counts.sum()) == vol.size, (name, bins)
                assert h.stats.sum == float(vol.astype(np.int64).sum()) and h.stats.sum_sq == float((vol.astype(np.int64) ** 2).sum())
            h = ctx.volume_histogram(16, (0.5, 0.75))  # categories on the collapsed path: the constant 93 / 255 lies below
            assert h.n_below == int((vol < 128).sum()) and h.n_above == int((vol > 191).sum()) and int(h.counts.sum()) == int(((vol >= 128) & (vol <= 191)).sum())
        finally:
            ctx.close()


def test_null_outputs(V, volumes):  # noqa: F811
    N = V.native
    ctx = _ctx(V, volumes["odd"])
    try:
        full = ctx.volume_histogram(64, (0.1, 0.9))
        req = N.VkHistogram(0.1, 0.9, 64, 0)
        counts = (C.c_uint64 * 64)()
        st = N.VkVolumeStats()
        assert N.lib().vk_volume_histogram(ctx.handle, C.byref(req), None, counts, None) == 0
        assert list(counts) == [int(v) for v in full.counts]
        assert N.lib().vk_volume_histogram(ctx.handle, C.byref(req), None, None, C.byref(st)) == 0
        assert (st.n_voxels, st.n_below, st.n_above, st.sum, st.sum_sq, st.min, st.max, st.scale) == (
            full.n_voxels, full.n_below, full.n_above, full.stats.sum, full.stats.sum_sq, full.stats.min, full.stats.max, 255.0)
        assert N.lib().vk_volume_histogram(ctx.handle, C.byref(req), None, None, None) == 0
    finally:
        ctx.close()


def _centres_box(lo, hi, dims):
    """The voxels whose centres (i + 0.5) / n lie in the closed f32 interval, by brute force in double."""
    out = []
    for a, b, n in zip(lo, hi, dims):
        a, b = float(np.float32(a)), float(np.float32(b))
        inside = [i for i in range(n) if a <= (i + 0.5) / n <= b]
        out.append((inside[0], inside[-1] + 1) if inside else (0, 0))
    return tuple(r[0] for r in out), tuple(r[1] for r in out)


@pytest.mark.parametrize("layout", ["LINEAR", "PACKED"])
def test_clip_box_flag_is_the_explicit_voxel_box(V, volumes, layout):  # noqa: F811
    vol = volumes["odd"]
    nz, ny, nx = vol.shape
    ctx = _ctx(V, vol, None, layout)
    try:
        whole = ctx.volume_histogram(256, (0.0, 1.0))
        assert not _same(ctx.volume_histogram(256, (0.0, 1.0), "clip"), whole, sums=True)  # no clip box set: the whole volume
        for lo, hi in (((0.2, 0.1, 0.0), (0.8, 0.9, 0.7)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.5 / nx, 0.25, 0.5 / nz), (1.5 / nx, 0.75, 1.0))):
            ctx.set_clip_box(lo, hi)
            box = _centres_box(lo, hi, (nx, ny, nz))
            want = ctx.volume_histogram(256, (0.0, 1.0), box)
            got = ctx.volume_histogram(256, (0.0, 1.0), "clip")
            sub = vol[box[0][2]:box[1][2], box[0][1]:box[1][1], box[0][0]:box[1][0]]
            assert not _same(got, want, sums=True) and got.n_voxels == sub.size > 0 and (got.counts == np.bincount(sub.ravel(), minlength=256).astype(np.uint64)).all(), (lo, hi)
            # the box and the flag together are refused
            code, msg = _code(V, lambda: V.native.check(ctx.handle, V.native.lib().vk_volume_histogram(
                ctx.handle, C.byref(V.VkHistogram(0.0, 1.0, 256, V.HIST_CLIP_BOX)), C.byref(V.VkVoxelBox(0, 0, 0, 1, 1, 1)), None, None)))
            assert code == INVALID and "box must be NULL" in msg
        # a clip box that contains no voxel centre: between the centres of voxels 3 and 4 of x
        lo, hi = (3.6 / nx, 0.0, 0.0), (4.4 / nx, 1.0, 1.0)
        ctx.set_clip_box(lo, hi)
        assert _centres_box(lo, hi, (nx, ny, nz))[0][0] == _centres_box(lo, hi, (nx, ny, nz))[1][0]
        h = ctx.volume_histogram(256, (0.0, 1.0), "clip")
        assert h.n_voxels == 0 and not h.counts.any() and h.stats.min == np.inf and h.stats.max == -np.inf and h.stats.sum == 0.0 and np.isnan(h.mean)
        ctx.set_clip_box(None)
        assert not _same(ctx.volume_histogram(256, (0.0, 1.0), "clip"), whole, sums=True)
    finally:
        ctx.close()


def test_the_pass_leaves_the_context_as_it_was(V, volumes):  # noqa: F811
    W, H = 48, 32
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, volumes["uniform"], layout=V.LAYOUT_PACKED)
        ctx.update()
        ctx.reset_step_counts()
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0, flags=V.RENDER_COUNT)
        pipe.record(ctx)
        before, steps, counts = ctx.read_backbuffer().copy(), ctx.read_steps().copy(), ctx.step_counts()
        assert np.abs(before[..., :3]).sum() > 0
        h = ctx.volume_histogram(512, (0.0, 1.0))
        assert int(h.counts.sum()) == volumes["uniform"].size
        assert (ctx.read_backbuffer().view(np.uint32) == before.view(np.uint32)).all() and (ctx.read_steps() == steps).all()
        assert ctx.step_counts() == counts
        ctx.reset_step_counts()
        pipe.record(ctx)
        assert (ctx.read_backbuffer().view(np.uint32) == before.view(np.uint32)).all() and ctx.step_counts() == counts
        # inside a frame: on the frame's stream, behind the render recorded there
        ctx.frames_in_flight(2)
        ctx.reset_step_counts()
        fid = ctx.frame_begin()
        pipe.record(ctx)
        inside = ctx.volume_histogram(512, (0.0, 1.0))
        ctx.frame_end()
        assert not _same(inside, h, sums=True)
        assert (ctx.read_frame(fid).view(np.uint32) == before.view(np.uint32)).all()
    finally:
        ctx.close()


def test_repeated_calls_do_not_leak_device_memory(V, volumes):  # noqa: F811
    import torch

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    ctx = _ctx(V, volumes["odd"])
    try:
        for i in range(8):
            ctx.volume_histogram(4096 if i % 2 else 7, (0.0, 1.0))
        before = free_bytes()
        for i in range(40):
            ctx.volume_histogram(4096 if i % 2 else 7, (0.0, 1.0), None if i % 3 else ((1, 1, 1), (9, 9, 5)))
        after = free_bytes()
        assert before - after < (2 << 20), f"{(before - after) / 2**20:.1f} MiB of device memory lost over 40 calls"
    finally:
        ctx.close()


def test_every_refusal_returns_its_status_and_leaves_the_outputs_alone(V, volumes):  # noqa: F811
    N = V.native
    vol = volumes["odd"]
    nz, ny, nx = vol.shape
    counts = (C.c_uint64 * 4096)()
    st = N.VkVolumeStats()

    def mark():
        for i in range(4096):
            counts[i] = 0xABCD
        st.n_voxels, st.sum = 123456789, -7.5

    def untouched():
        return all(counts[i] == 0xABCD for i in (0, 1, 255, 4095)) and st.n_voxels == 123456789 and st.sum == -7.5

    def raw(ctx, req, box=None):
        mark()
        rc = N.lib().vk_volume_histogram(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None, counts, C.byref(st))
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    ctx = _ctx(V, vol)
    try:
        refused = [(None, None, "NULL")]
        for bins in (0, 4097, 1 << 31):
            refused.append((N.VkHistogram(0.0, 1.0, bins, 0), None, "bins"))
        for lo, hi in ((float("nan"), 1.0), (0.0, float("inf")), (-float("inf"), 0.0), (1.0, 1.0), (0.5, 0.25)):
            refused.append((N.VkHistogram(lo, hi, 16, 0), None, "lo and hi"))
        for flags in (2, 4, 3, 1 << 31):
            refused.append((N.VkHistogram(0.0, 1.0, 16, flags), None, "flag"))
        for box in ((2, 0, 0, 1, 1, 1), (0, 3, 0, 1, 2, 1), (0, 0, 0, nx + 1, 1, 1), (0, 0, 0, 1, ny + 1, 1), (0, 0, nz, 1, 1, nz + 1), (0, 0, 0, 0xffffffff, 1, 1)):
            refused.append((N.VkHistogram(0.0, 1.0, 16, 0), N.VkVoxelBox(*box), "inverted or leaves the volume"))
        refused.append((N.VkHistogram(0.0, 1.0, 16, N.HIST_CLIP_BOX), N.VkVoxelBox(0, 0, 0, 1, 1, 1), "box must be NULL"))
        for req, box, word in refused:
            rc, msg = raw(ctx, req, box)
            assert rc == INVALID and word in msg and untouched(), (word, rc, msg)
        # what is accepted: an empty box anywhere inside, on the far corner too
        for box in ((3, 3, 3, 3, 3, 3), (nx, ny, nz, nx, ny, nz), (0, 0, 0, nx, 0, nz)):
            rc, msg = raw(ctx, N.VkHistogram(0.0, 1.0, 16, 0), N.VkVoxelBox(*box))
            assert rc == 0 and st.n_voxels == 0 and st.min == np.inf and st.max == -np.inf and st.sum == 0.0 and not any(counts[i] for i in range(16)) and counts[16] == 0xABCD
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, None, layout)
        try:
            rc, msg = raw(ctx, N.VkHistogram(0.0, 1.0, 16, 0))
            assert rc == UNSUPPORTED and "histogram" in msg and untouched(), layout
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, N.VkHistogram(0.0, 1.0, 16, 0))
        assert rc == UNSUPPORTED and "histogram" in msg and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, N.VkHistogram(0.0, 1.0, 16, 0))
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()


@pytest.mark.parametrize("kind, layout", SEVEN)
def test_python_mean_std_and_window_against_numpy(V, volumes, kind, layout):  # noqa: F811
    vol = {"u8": volumes["odd"], "u16": volumes["passes"][:9, :21, :35], "f16": volumes["f16"]}[kind]
    vol = np.ascontiguousarray(vol)
    scale = NH.SCALE[kind]
    x = vol.astype(np.float64) / scale
    lo, hi = (0.0, 1.0) if kind != "f16" else (-1.0, 2.0)
    ctx = _ctx(V, vol, kind, layout)
    try:
        h = ctx.volume_histogram(200, (lo, hi))
        assert h.n_finite == vol.size
        assert abs(h.mean - x.mean()) <= 1e-12 * max(1.0, abs(x.mean())) and abs(h.std - x.std()) <= 1e-9 * max(1.0, x.std())
        assert h.min == x.min() and h.max == x.max()
        assert h.edges[0] == lo and h.edges[-1] == hi and len(h.edges) == 201
        # the window of the 5th .. 95th percentile: the bins of the sorted samples at those ranks
        inr = np.sort(np.clip(np.floor((x[(x >= lo) & (x <= hi)] - lo) * 200 / (hi - lo)), 0, 199).astype(np.int64))
        n = int(h.counts.sum())
        assert n == inr.size or kind == "f16"  # (integer data: the float64 bins above are the kernel's, bincount-exact; f16: the counts decide)
        cum = np.cumsum(h.counts.astype(np.int64))
        b_lo = int(np.argmax(cum > np.floor(0.05 * n)))
        b_hi = max(int(np.argmax(cum >= np.ceil(0.95 * n))), b_lo)
        w = h.window(0.05, 0.95)
        assert w == (float(np.float32(lo + b_lo * (hi - lo) / 200)), float(np.float32(lo + (b_hi + 1) * (hi - lo) / 200)))
        assert lo <= w[0] < w[1] <= hi
        with pytest.raises(V.VokselisError):
            h.window(0.9, 0.1)
    finally:
        ctx.close()


def test_window_of_a_known_histogram(V):  # noqa: F811
    vol = np.zeros((4, 4, 4), np.uint8)
    vol.ravel()[:16] = 100   # 16 voxels of 100, 48 of 0
    vol.ravel()[16:20] = 250
    ctx = _ctx(V, vol, "u8", "LINEAR")
    try:
        h = ctx.volume_histogram(256, (0.0, 1.0))
        assert int(h.counts[0]) == 44 and int(h.counts[100]) == 16 and int(h.counts[250]) == 4
        assert h.window(0.0, 1.0) == (0.0, float(np.float32(251 / 256)))
        assert h.window(0.75, 0.9) == (float(np.float32(100 / 256)), float(np.float32(101 / 256)))  # ranks 48 .. 58 of 64: all in bin 100
        assert h.window(0.0, 0.5) == (0.0, float(np.float32(1 / 256)))
    finally:
        ctx.close()
