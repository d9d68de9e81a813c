"""vk_extract_isosurface on the MI355X through its entry point: the multi-chunk, grid-stride and compaction paths under
mesh_chunk_cubes and mesh_max_blocks, the count-only call, truncation to an exact prefix with the memory behind it untouched,
VK_MESH_CLIP_BOX against the explicit box, a constant volume, the state the pass must leave alone, a call inside a frame, device memory over
repeated calls, every refusal with its status, and one cross-check against the renderer: on an affine volume the geometry pass's hits lie on
the mesh's plane.  The kernels are held to the restatement over the shared cases in tests/test_mesh_fuzz_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import mesh_helpers as MH
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
KIND = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float16): "f16"}


def _ctx(V, vol, layout="PACKED", size=(32, 24), camera=None):
    ctx = V.Context(size[0], size[1], camera, backbuffer=size, out_format=V.OUT_RGBA32F)
    try:
        if vol is not None:
            MH.upload(V, ctx, vol, KIND[vol.dtype], layout)
    except BaseException:
        ctx.close()
        raise
    return ctx


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return MH.build_restatement(tmp_path_factory.mktemp("mesh_gpu"))


@pytest.fixture(scope="module")
def volumes():
    rng = np.random.default_rng(12)
    z, y, x = np.meshgrid((np.arange(40) + 0.5) / 40 * 2 - 1, (np.arange(64) + 0.5) / 64 * 2 - 1, (np.arange(64) + 0.5) / 64 * 2 - 1, indexing="ij")
    ball = np.rint(np.clip(1.3 - 1.6 * np.sqrt(x * x + y * y + z * z), 0.0, 1.0) * 255).astype(np.uint8)
    speckle = rng.random(ball.shape) < 0.002
    ball[speckle] = 255 - ball[speckle]       # lone voxels inside and outside: chunks with one or two live cubes between empty ones
    v = {"odd": rng.integers(0, 256, (7, 20, 33)).astype(np.uint8),   # 33 x 20 x 7
         "ball": ball,                                                # 64 x 64 x 40: 155 k cubes, most of them empty
         "ball16": (ball.astype(np.uint16) * 257),
         "constant": np.full((24, 24, 24), 93, np.uint8)}
    for a in v.values():
        a.setflags(write=False)
    return v


@pytest.mark.parametrize("name, layouts", [("odd", ("LINEAR", "PACKED", "PACKED_PAIRS")), ("ball", ("LINEAR", "PACKED_PAIRS")), ("ball16", ("PACKED",))])
def test_small_chunks_and_capped_grids_give_the_unconstrained_result(V, lib, volumes, name, layouts):  # noqa: F811
    vol = volumes[name]
    nz, ny, nx = vol.shape
    box = ((1, 0, 1), (nx, ny - 1, nz))
    for layout in layouts:
        ctx = _ctx(V, vol, layout)
        try:
            for b in (None, box):
                free = ctx.extract_isosurface(0.5, b)
                assert MH.same_bits(free, MH.restate(lib, vol, KIND[vol.dtype], 0.5, b)) and len(free) > 5000
                for chunk in (64, 256):
                    for blocks in (1, 2, 3):
                        ctx.set_param("mesh_chunk_cubes", chunk)
                        ctx.set_param("mesh_max_blocks", blocks)
                        assert MH.same_bits(ctx.extract_isosurface(0.5, b), free), (layout, b, chunk, blocks)
                ctx.set_param("mesh_chunk_cubes", 4096)
                ctx.set_param("mesh_max_blocks", 0)
                assert MH.same_bits(ctx.extract_isosurface(0.5, b), free), (layout, b, 4096)
                ctx.set_param("mesh_chunk_cubes", 0)
                assert MH.same_bits(ctx.extract_isosurface(0.5, b), free)
        finally:
            ctx.close()


def _raw(V, ctx, iso, triangles, cap, box=None, flags=0):
    N = V.native
    n = C.c_uint64(0xDEADBEEF)
    req = N.VkMeshRequest(iso, flags)
    ptr = triangles.ctypes.data_as(C.POINTER(C.c_float)) if triangles is not None else None
    rc = N.lib().vk_extract_isosurface(ctx.handle, C.byref(req), C.byref(box) if box is not None else None, ptr, cap, C.byref(n))
    return rc, int(n.value)


@pytest.mark.parametrize("layout", ["LINEAR", "PACKED"])
def test_count_only_and_truncation_to_an_exact_prefix(V, lib, volumes, layout):  # noqa: F811
    vol = volumes["odd"]
    full = MH.restate(lib, vol, "u8", 0.5)
    n = len(full)
    ctx = _ctx(V, vol, layout)
    try:
        assert _raw(V, ctx, 0.5, None, 0) == (0, n) and _raw(V, ctx, 0.5, None, 1 << 40) == (0, n)
        canary = np.float32(-12345.5)
        for chunk in (0, 64):
            ctx.set_param("mesh_chunk_cubes", chunk)
            for cap in (0, 1, n - 1, n, n + 5):
                buf = np.full((n + 8, 3, 3), canary, np.float32)
                assert _raw(V, ctx, 0.5, buf, cap) == (0, n), cap
                m = min(cap, n)
                assert MH.same_bits(buf[:m], full[:m]) and (buf[m:] == canary).all(), (chunk, cap)
        assert MH.same_bits(ctx.extract_isosurface(0.5, max_triangles=17), full[:17])
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
def test_clip_box_flag_is_the_explicit_voxel_box(V, lib, volumes, layout):  # noqa: F811
    vol = volumes["odd"]
    nz, ny, nx = vol.shape
    ctx = _ctx(V, vol, layout)
    try:
        whole = ctx.extract_isosurface(0.5)
        assert MH.same_bits(ctx.extract_isosurface(0.5, "clip"), whole) and len(whole) > 0  # no clip box set: the whole volume
        for lo, hi in (((0.2, 0.1, 0.0), (0.8, 0.9, 0.7)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.5 / nx, 0.25, 0.5 / nz), (2.5 / nx, 0.75, 1.0))):
            ctx.set_clip_box(lo, hi)
            box = _centres_box(lo, hi, (nx, ny, nz))
            got = ctx.extract_isosurface(0.5, "clip")
            assert MH.same_bits(got, ctx.extract_isosurface(0.5, box)) and MH.same_bits(got, MH.restate(lib, vol, "u8", 0.5, box)) and len(got) > 0, (lo, hi)
            rc, n = _raw(V, ctx, 0.5, None, 0, V.VkVoxelBox(0, 0, 0, 2, 2, 2), V.MESH_CLIP_BOX)  # the box and the flag together are refused
            assert rc == INVALID and n == 0xDEADBEEF and b"box must be NULL" in V.native.lib().vk_last_error(ctx.handle)
        ctx.set_clip_box((3.6 / nx, 0.0, 0.0), (4.4 / nx, 1.0, 1.0))  # no voxel centre inside
        assert len(ctx.extract_isosurface(0.5, "clip")) == 0
        ctx.set_clip_box(None)
        assert MH.same_bits(ctx.extract_isosurface(0.5, "clip"), whole)
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", ["LINEAR", "PACKED", "PACKED_PAIRS"])
def test_constant_volume_has_no_triangles(V, volumes, layout):  # noqa: F811
    """Every chunk total is 0: n == 0 leaves nothing to write, and the emit pass is not launched (the buffer keeps its canary)."""
    ctx = _ctx(V, volumes["constant"], layout)
    try:
        for iso in (0.1, 93.0 / 255.0, 0.9):  # all inside, at the value, all outside
            buf = np.full((4, 3, 3), np.float32(7.25), np.float32)
            assert _raw(V, ctx, iso, buf, 4) == (0, 0) and (buf == np.float32(7.25)).all()
            assert ctx.extract_isosurface(iso).shape == (0, 3, 3)
    finally:
        ctx.close()


def test_the_pass_leaves_the_context_as_it_was(V, lib, volumes):  # noqa: F811
    W, H = 48, 32
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    vol = volumes["ball"]
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        V.VolumeTexture(ctx, vol, layout=V.LAYOUT_PACKED)
        ctx.update()
        ctx.set_isosurface(0.3, (1.0, 0.5, 0.25), 5)
        ctx.reset_step_counts()
        pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0, flags=V.RENDER_COUNT)
        pipe.record(ctx)
        before, steps, counts = ctx.read_backbuffer().copy(), ctx.read_steps().copy(), ctx.step_counts()
        maps = ctx.read_skip_maps()
        assert np.abs(before[..., :3]).sum() > 0
        want = MH.restate(lib, vol, "u8", 0.5)
        assert MH.same_bits(ctx.extract_isosurface(0.5), want) and len(want) > 1000   # another isovalue than the stored one
        assert (ctx.read_backbuffer().view(np.uint32) == before.view(np.uint32)).all() and (ctx.read_steps() == steps).all()
        assert ctx.step_counts() == counts and ctx.isosurface == (np.float32(0.3), (1.0, 0.5, 0.25), 5)
        after = ctx.read_skip_maps()
        assert after[0] == maps[0] and maps[1].size > 0 and np.array_equal(after[1], maps[1])
        ctx.reset_step_counts()
        pipe.record(ctx)
        assert (ctx.read_backbuffer().view(np.uint32) == before.view(np.uint32)).all() and ctx.step_counts() == counts
        # inside a frame: on the frame's stream, behind the render recorded there
        ctx.frames_in_flight(2)
        ctx.reset_step_counts()
        fid = ctx.frame_begin()
        pipe.record(ctx)
        inside = ctx.extract_isosurface(0.5)
        ctx.frame_end()
        assert MH.same_bits(inside, want)
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
            ctx.extract_isosurface(0.5 if i % 2 else 0.25)
        before = free_bytes()
        for i in range(40):
            ctx.extract_isosurface(0.5 if i % 2 else 0.25, None if i % 3 else ((1, 1, 1), (9, 9, 5)))
        after = free_bytes()
        assert before - after < (2 << 20), f"{(before - after) / 2**20:.1f} MiB of device memory lost over 40 calls"
    finally:
        ctx.close()


def test_every_refusal_returns_its_status_and_leaves_the_outputs_alone(V, volumes):  # noqa: F811
    N = V.native
    vol = volumes["odd"]
    nz, ny, nx = vol.shape
    buf = np.zeros((16, 3, 3), np.float32)
    n = C.c_uint64(0)

    def raw(ctx, req, box=None, n_ptr=True):
        buf[:] = np.float32(-3.5)
        n.value = 987654321
        rc = N.lib().vk_extract_isosurface(ctx.handle, C.byref(req) if req is not None else None, C.byref(box) if box is not None else None,
                                           buf.ctypes.data_as(C.POINTER(C.c_float)), 16, C.byref(n) if n_ptr else None)
        return rc, N.lib().vk_last_error(ctx.handle).decode()

    def untouched():
        return bool((buf == np.float32(-3.5)).all()) and n.value == 987654321

    ctx = _ctx(V, vol)
    try:
        refused = [(None, None, "NULL")]
        for iso in (float("nan"), float("inf"), -float("inf")):
            refused.append((N.VkMeshRequest(iso, 0), None, "finite"))
        for flags in (2, 4, 3, 1 << 31):
            refused.append((N.VkMeshRequest(0.5, flags), None, "flag"))
        for box in ((2, 0, 0, 1, 1, 1), (0, 3, 0, 1, 2, 1), (0, 0, 0, nx + 1, 1, 1), (0, 0, 0, 1, ny + 1, 1), (0, 0, nz, 1, 1, nz + 1), (0, 0, 0, 0xffffffff, 1, 1)):
            refused.append((N.VkMeshRequest(0.5, 0), N.VkVoxelBox(*box), "inverted or leaves the volume"))
        refused.append((N.VkMeshRequest(0.5, N.MESH_CLIP_BOX), N.VkVoxelBox(0, 0, 0, 1, 1, 1), "box must be NULL"))
        for req, box, word in refused:
            rc, msg = raw(ctx, req, box)
            assert rc == INVALID and "vk_extract_isosurface" in msg and word in msg and untouched(), (word, rc, msg)
        rc, msg = raw(ctx, N.VkMeshRequest(0.5, 0), None, n_ptr=False)
        assert rc == INVALID and "n_triangles" in msg and untouched()
        # what is accepted: an empty or thin box anywhere inside, on the far corner too -- 0 triangles
        for box in ((3, 3, 3, 3, 3, 3), (nx, ny, nz, nx, ny, nz), (0, 0, 0, nx, 1, nz)):
            rc, msg = raw(ctx, N.VkMeshRequest(0.5, 0), N.VkVoxelBox(*box))
            assert rc == 0 and n.value == 0 and bool((buf == np.float32(-3.5)).all())
    finally:
        ctx.close()
    for layout in ("BRICKED", "QUADS", "STAGED"):
        ctx = _ctx(V, vol, layout)
        try:
            rc, msg = raw(ctx, N.VkMeshRequest(0.5, 0))
            assert rc == UNSUPPORTED and msg.startswith("mesh: ") and untouched(), layout
        finally:
            ctx.close()
    ctx = V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)  # an RGBA16F_PAIR volume
    try:
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16))
        rc, msg = raw(ctx, N.VkMeshRequest(0.5, 0))
        assert rc == UNSUPPORTED and msg.startswith("mesh: ") and untouched()
    finally:
        ctx.close()
    ctx = _ctx(V, None)  # no volume
    try:
        rc, msg = raw(ctx, N.VkMeshRequest(0.5, 0))
        assert rc == INVALID and "no volume" in msg and untouched()
    finally:
        ctx.close()


@pytest.mark.parametrize("layout", ["LINEAR", "PACKED"])
def test_the_renderers_hits_lie_on_the_meshs_plane(V, layout):  # noqa: F811
    """A volume whose texels are an affine function of position, V(i, j, k) = 20 + 3 i + 2 j + k: linear interpolation over tetrahedra and the
    trilinear filter both reproduce it exactly in real arithmetic, so the mesh and the render's surface are the same plane
    20 + 3 (n x - 0.5) + 2 (n y - 0.5) + (n z - 0.5) = iso_k, |gradient| = n sqrt(14) per unit of the cube.

    Bounds, derived from the roundings, not tuned.
    Mesh: f is one subtraction of small integers from a half-integer (exact), one division; a coordinate is two additions and a division of
    numbers below 2^5: 4 roundings of relative size 2^-24 on coordinates <= 1 -> |d pos| <= 4 * 2^-24 per axis, and the distance from the
    plane at most sqrt(3) times that.
    Render: the geometry pass ends its bisection with a computed sample >= iso_k at q and a computed sample < iso_k one step of 2^-R |s|
    nearer the eye (R = 16, |s| = dt <= sqrt(3) / n).  The filter is 7 lerps, each a subtraction and an fma on values < 256 (half an ulp of
    2^-16 each: 14 * 2^-17), on fractions whose own error -- a coordinate * n - 0.5, 2 roundings at 2^-24 * n -- moves the value by the
    slope, at most 3 + 2 + 1 per voxel: 6 * 2 * 2^-24 * n.  So the signed distance of q from the plane lies in
    [-eps_T / |g|, eps_T / |g| + 2^-R sqrt(3) / n], widened by 3 * 2^-24 for q's own roundings.
    Hits nearer than 3 voxels to a face are left out: there the filter clamps its indices and is no longer affine along the last step."""
    n = 40  # (20 + 6 * 39 = 254: the largest texel still fits a u8)
    k, j, i = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    vol = (20 + 3 * i + 2 * j + k).astype(np.uint8)
    iso_k = np.float32(0.5) * np.float32(255.0)  # 127.5
    W, H = 192, 144
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    ctx = _ctx(V, vol, layout, (W, H), cam)
    try:
        ctx.update()
        tris = ctx.extract_isosurface(0.5)
        assert len(tris) > 500
        g = np.array([3.0, 2.0, 1.0]) * n
        glen = float(np.sqrt((g * g).sum()))

        def distance(p):  # signed, towards higher values
            v = 20.0 + (p.astype(np.float64) * n - 0.5) @ np.array([3.0, 2.0, 1.0])
            return (v - float(iso_k)) / glen

        eps_mesh = np.sqrt(3.0) * 4 * 2.0 ** -24
        d_mesh = distance(tris.reshape(-1, 3))
        assert np.abs(d_mesh).max() <= eps_mesh, (float(np.abs(d_mesh).max()), eps_mesh)
        # every triangle's normal is the plane's outward normal -g / |g| (zero-area triangles aside)
        nrm = MH.normals(tris)
        big = np.sqrt((nrm * nrm).sum(axis=1)) > 1e-9
        assert big.sum() > 500 and ((nrm[big] @ (-g / glen)) / np.sqrt((nrm[big] * nrm[big]).sum(axis=1)) > 1.0 - 1e-6).all()

        R = 16
        ctx.set_isosurface(0.5, refine=R)
        ctx.render_geometry(1.0)
        pos_t, grad_x = ctx.read_geometry()
        hit = np.isfinite(pos_t[..., 3])
        q = pos_t[..., :3]
        interior = hit & (q >= 3.0 / n).all(axis=-1) & (q <= 1.0 - 3.0 / n).all(axis=-1)
        assert interior.sum() > 200, int(interior.sum())
        eps_t = 14 * 2.0 ** -17 + 6 * 2 * 2.0 ** -24 * n
        lo = -eps_t / glen - 3 * 2.0 ** -24 - eps_mesh
        hi = eps_t / glen + 2.0 ** -R * np.sqrt(3.0) / n + 3 * 2.0 ** -24 + eps_mesh
        d = distance(q[interior])
        print(f"\n{layout}: {int(interior.sum())} interior hits, distance from the mesh's plane in [{d.min():.3g}, {d.max():.3g}], allowed [{lo:.3g}, {hi:.3g}]")
        assert d.min() >= lo and d.max() <= hi
        ys, xs = np.nonzero(interior)
        for y, x in list(zip(ys, xs))[:: max(1, len(ys) // 4)][:4]:  # vk_pick is the pass's record of the pixel
            p = ctx.pick(int(x), int(y), 1.0)
            assert p is not None and lo <= distance(np.array(p.pos, np.float32)) <= hi
    finally:
        ctx.close()
