"""Every allocation of every entry point, made to fail: vk_debug_set_param(ctx, "alloc_fail_at", k) fails the k-th
allocation a context makes, and a row of tests/alloc_failure_cases.py is swept over k = 1, 2, ... until its call returns VK_OK.  After
every failing call: VK_ERR_OOM, the entry's prefix and a buffer's name in the message, the context's volume, maps, projection, isosurface
and 64 x 64 frame as before the call, every output buffer wholly untouched or wholly the result; after the last: the call succeeds, its
outputs are the restatement's bit for bit, and an INSTALL has left what a fresh context holds after uploading the restatement's output.
The number of allocations a row made is pinned (AC.COUNTS) and so is the number of failing calls: an empty loop cannot pass.

The failing allocation is a real one: the library asks the runtime for 2^60 bytes, which it refuses at once (test_the_hooks_request_...
holds that first).  Nothing is exhausted, and no test here asks for more than a small volume's buffers."""
import ctypes as C
import time

import numpy as np
import pytest

import alloc_failure_cases as AC
import label_cases as LC
import label_helpers as LH
from gpu_helpers import V  # noqa: F401
from alloc_failure_cases import VK_ERR_INVALID, VK_ERR_OOM, VK_OK, H, W

pytestmark = pytest.mark.gpu

OOM = AC.OOM_TEXT
HELPERS = {"hist": "hist_helpers", "mesh": "mesh_helpers", "filter": "filter_helpers", "label": "label_helpers", "dist": "dist_helpers", "resample": "resample_helpers",
           "split": "split_helpers", "measure": "measure_helpers", "thick": "thick_helpers", "geo": "geo_helpers", "skel": "skel_helpers"}


class Env:
    """What the rows share: the package, the restatements (built once each) and their outputs (computed once each, left unchanged)."""

    def __init__(self, V, tmp):  # noqa: F811
        self.V, self.N, self.tmp = V, V.native, tmp
        self._libs, self._expected, self.summary = {}, {}, []

    def restatement(self, name):
        if name not in self._libs:
            self._libs[name] = __import__(HELPERS[name]).build_restatement(self.tmp.mktemp("alloc_failure_" + name))
        return self._libs[name]

    def expected(self, key, make):
        if key not in self._expected:
            e = make()
            for a in (e if isinstance(e, tuple) else (e,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._expected[key] = e
        return self._expected[key]


@pytest.fixture(scope="module")
def E(V, tmp_path_factory):  # noqa: F811
    env = Env(V, tmp_path_factory)
    yield env
    print("\nallocation-failure sweep: row, allocations (pinned), failing calls made")
    for line in env.summary:
        print("  " + line)


# ---- contexts, volumes, what a context holds --------------------------------------------------------------------------------------------
def new_ctx(E, slots=1):
    V = E.V  # noqa: F811
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        if slots > 1:
            ctx.frames_in_flight(slots)
        ctx.update()
    except BaseException:
        ctx.close()
        raise
    return ctx


def _pair():
    rng = np.random.default_rng(23)
    d = rng.uniform(0.0, 1.0, (9, 17, 33, 4)).astype(np.float16)
    n = rng.uniform(-1.0, 1.0, (9, 17, 33, 4)).astype(np.float16)
    return d, n


VOLUMES = {
    "u8": lambda: LC.noise((37, 21, 11), "u8", 80),                 # next to no empty cell: one isotropic map
    "u8 sparse": lambda: LC.blocks((37, 21, 11), "u8", "edge"),    # nearly all cells empty: the eight octant maps
    "u16": lambda: LC.noise((37, 21, 11), "u16", 80),
    "f16": lambda: LC.noise((37, 21, 11), "f16", 80),
    "old": lambda: LC.checkerboard((35, 10, 9), "u8"),              # the volume a build replaces
}


def volume(E, name):
    return E.expected(("volume", name), _pair if name == "pair" else VOLUMES[name])


def upload(E, ctx, name, layout):
    V = E.V  # noqa: F811
    if name == "pair":
        d, n = volume(E, name)
        return V.VolumeTexture(ctx, d, n, layout=getattr(V, "LAYOUT_" + layout))
    return LH.upload(V, ctx, volume(E, name), name.split()[0] if name != "old" else "u8", layout)


def last_error(E, ctx):
    return E.N.lib().vk_last_error(ctx.handle).decode()


def arm(ctx, k):
    ctx.set_param("alloc_fail_at", k)


def frame_of(E, ctx, fmt=None):
    """The 64 x 64 frame under the state in force (the compute mode for a pair volume, which has no trilinear march)."""
    N, L = E.N, E.N.lib()
    if fmt is None:
        f = C.c_int()
        N.check(ctx.handle, L.vk_volume_info(ctx.handle, None, C.byref(f), None, None))
        fmt = f.value
    N.check(ctx.handle, L.vk_backbuffer_clear(ctx.handle))
    N.check(ctx.handle, L.vk_render(ctx.handle, N.MODE_COMPUTE_NEAREST if fmt == N.FMT_RGBA16F_PAIR else N.MODE_NAIVE_TRILINEAR, 0, 0, W, H, 1.0, 0))
    return ctx.read_backbuffer().tobytes()


STATE = ("dims", "format", "layout", "device bytes", "empty fraction", "projection", "isosurface", "map grid", "skip maps", "frame")


def state(E, ctx):
    """What a failed call must leave as it was: vk_volume_info, vk_volume_empty_fraction, vk_get_projection, vk_get_isosurface, the skip
    maps' bytes and the frame -- or, without a volume, that there is none."""
    L = E.N.lib()
    dims, fmt, lay, nbytes = (C.c_uint32 * 3)(), C.c_int(), C.c_int(), C.c_size_t()
    rc = L.vk_volume_info(ctx.handle, dims, C.byref(fmt), C.byref(lay), C.byref(nbytes))
    if rc != VK_OK:
        return ("no volume", rc, last_error(E, ctx), ctx.projection, ctx.isosurface)
    ef = C.c_double(-1.0)
    E.N.check(ctx.handle, L.vk_volume_empty_fraction(ctx.handle, C.byref(ef)))
    grid, maps = ctx.read_skip_maps()
    return (tuple(dims), fmt.value, lay.value, nbytes.value, ef.value, ctx.projection, ctx.isosurface, grid, maps.tobytes(), frame_of(E, ctx, fmt.value))


def state_differences(a, b):
    if a == b:
        return ""
    if a[0] == "no volume" or b[0] == "no volume":
        return f"{a[:5]} != {b[:5]}"
    return ", ".join(n for n, x, y in zip(STATE, a, b) if x != y) + " changed"


NO_VOLUME = ("no volume", VK_ERR_INVALID, "no volume uploaded", None, None)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
def sweep(E, row, ctx, call, message_ok, before_call=None, after_call=None):
    """Arm at k = 1, 2, ...; call; until VK_OK.  Returns (failing calls as (k, message, outputs), the successful call's outputs)."""
    before = state(E, ctx)
    fails = []
    for k in range(1, 66):
        if before_call:
            before_call()
        arm(ctx, k)
        rc, outs = call()
        msg = last_error(E, ctx)
        arm(ctx, 0)
        if after_call:
            after_call(rc)
        if rc == VK_OK:
            break
        assert rc == VK_ERR_OOM, (row.id, k, rc, msg)
        assert msg.endswith(": " + OOM) and message_ok(msg), (row.id, k, msg)
        assert state_differences(state(E, ctx), before) == "", (row.id, k, msg)
        fails.append((k, msg, outs))
    else:
        raise AssertionError(f"{row.id}: still failing at k = 65")
    n = len(fails)
    E.summary.append(f"{row.id}: {n} allocations ({AC.COUNTS[row.id]}), {n} failing calls")
    assert [f[0] for f in fails] == list(range(1, n + 1)) and 1 <= n <= 64
    assert n == AC.COUNTS[row.id], (row.id, n, [f[1] for f in fails])
    return fails, outs


def rows(group):
    return [pytest.param(r, id=r.id) for r in AC.ROWS if r.group == group]


# ---- first of all: the request the hook makes -------------------------------------------------------------------------------------------
def test_the_hooks_request_is_refused_at_once_and_takes_nothing(E):
    """vk_device_alloc with the hook armed: VK_ERR_OOM within a millisecond-scale bound, the pointer NULL, the device's free memory as it
    was, the hook disarmed by having fired.  Everything else in this file rests on it."""
    import torch

    row = next(r for r in AC.ROWS if r.id == "vk_device_alloc")
    L = E.N.lib()
    ctx = new_ctx(E)
    try:
        torch.cuda.synchronize()
        free = torch.cuda.mem_get_info()
        arm(ctx, 1)
        p = C.c_void_p(0x1234)
        t0 = time.perf_counter()
        rc = L.vk_device_alloc(ctx.handle, 4096, C.byref(p))
        dt = time.perf_counter() - t0
        assert (rc, last_error(E, ctx), p.value) == (VK_ERR_OOM, "vk_device_alloc: " + OOM, None)
        assert dt < 0.25, dt
        assert torch.cuda.mem_get_info() == free
        arm(ctx, 2)  # the second from now on: the first passes
        q, r = C.c_void_p(), C.c_void_p(0x1234)
        assert L.vk_device_alloc(ctx.handle, 4096, C.byref(q)) == VK_OK and q.value
        assert L.vk_device_alloc(ctx.handle, 4096, C.byref(r)) == VK_ERR_OOM and r.value is None
        assert L.vk_device_alloc(ctx.handle, 4096, C.byref(r)) == VK_OK and r.value  # it fired: disarmed
        arm(ctx, 1)
        arm(ctx, 0)  # disarmed by hand
        s = C.c_void_p()
        assert L.vk_device_alloc(ctx.handle, 4096, C.byref(s)) == VK_OK and s.value
        for ptr in (q, r, s):
            assert L.vk_device_free(ctx.handle, ptr) == VK_OK
        assert L.vk_debug_set_param(ctx.handle, b"alloc_fail_at", -1.0) == VK_ERR_INVALID
        E.summary.append(f"{row.id}: 1 allocations ({AC.COUNTS[row.id]}), 1 failing calls")
        assert AC.COUNTS[row.id] == 1
    finally:
        ctx.close()


# ---- volume builds -----------------------------------------------------------------------------------------------------------------------
def _build_call(E, ctx, how, vol, lay, keep):
    """The call of a build row; keep: what must stay alive while the calls are made (device tensors)."""
    import torch

    N, L = E.N, E.N.lib()
    layout = getattr(N, "LAYOUT_" + lay)
    if how == "generate":
        fmt, kind = (N.FMT_R8_UNORM, N.GEN_BONSAI_STANDIN) if vol == "u8" else (N.FMT_R16_FLOAT, N.GEN_FOG)
        return lambda: (L.vk_volume_generate(ctx.handle, kind, 33, 17, 9, fmt, 0x5EED0001, 20, 12, layout), [])
    if how == "generate_xor":
        return lambda: (L.vk_volume_generate_xor(ctx.handle, 33, 17, 9, 0.5), [])
    arrays = volume(E, vol) if vol == "pair" else (volume(E, vol), None)
    nz, ny, nx = arrays[0].shape[:3]
    fmt = N.FMT_RGBA16F_PAIR if vol == "pair" else {"u8": N.FMT_R8_UNORM, "u16": N.FMT_R16_UNORM, "f16": N.FMT_R16_FLOAT}[vol.split()[0]]
    if how == "upload":
        ptrs = [a.ctypes.data if a is not None else None for a in arrays]
        return lambda: (L.vk_volume_upload(ctx.handle, ptrs[0], ptrs[1], nx, ny, nz, fmt, layout), [])
    for a in arrays:
        keep.append(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() if a is not None else None)
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() if t is not None else None for t in keep[-2:]]
    return lambda: (L.vk_volume_upload_device(ctx.handle, ptrs[0], ptrs[1], nx, ny, nz, fmt, layout), [])


BUILD_OWN = {"vk_volume_upload": ("volume upload: dense source: " + OOM, "volume upload: dense source (normals): " + OOM), "vk_volume_upload_device": (),
             "vk_volume_generate": ("generator: dense volume: " + OOM,), "vk_volume_generate_xor": ("xor generator: density: " + OOM, "xor generator: normals: " + OOM)}


@pytest.mark.parametrize("row", rows("build"))
def test_a_failed_build_leaves_the_volume_that_was(E, row):
    how, vol, lay, over = row.what
    keep = []
    ctx, ref = new_ctx(E), new_ctx(E)
    try:
        if over:
            upload(E, ctx, "old", "PACKED_PAIRS")
        else:
            assert state(E, ctx) == NO_VOLUME
        allowed = AC.BUILD_MESSAGES + BUILD_OWN[row.entry]
        fails, _ = sweep(E, row, ctx, _build_call(E, ctx, how, vol, lay, keep), lambda m: m in allowed)
        if BUILD_OWN[row.entry]:  # the first allocation is the entry's own: the dense source
            assert fails[0][1] == BUILD_OWN[row.entry][0], fails[0][1]
        # the build that went through is the build of a context that never failed
        rc, _ = _build_call(E, ref, how, vol, lay, keep)()
        assert rc == VK_OK, last_error(E, ref)
        got, want = state(E, ctx), state(E, ref)
        assert state_differences(got, want) == "" and got[0] != "no volume", row.id
        if (vol, lay) in (("u8", "PACKED"), ("u8 sparse", "PACKED")):  # both branches of the maps' build: one map, eight octants
            n_maps = len(got[8]) // (got[7][0] * got[7][1] * got[7][2])
            assert (n_maps, got[4] >= 0.30) == ((8, True) if vol == "u8 sparse" else (1, False)), (n_maps, got[4])
    finally:
        ctx.close()
        ref.close()


# ---- setters that rebuild the maps ---------------------------------------------------------------------------------------------------------
def _table(E):
    return E.V.transfer_table([(0.0, 0, 0, 0, 0), (0.4, 0, 0, 0, 0), (0.6, 1.0, 0.5, 0.2, 0.8), (1.0, 1, 1, 1, 1)], 64)


def _setter(E, ctx, entry, step):
    """(what brings the context to where the step starts, the step as a raw call)."""
    N, L = E.N, E.N.lib()
    t = _table(E)
    iso = lambda v: N.VkIsosurface(v, (C.c_float * 3)(0.9, 0.8, 0.7), 4)  # noqa: E731
    if entry == "vk_set_transfer_function":
        if step == "set":
            return (lambda: None), (lambda: (L.vk_set_transfer_function(ctx.handle, t.ctypes.data_as(C.POINTER(C.c_float)), len(t), 0.0, 1.0), []))
        return (lambda: ctx.set_transfer_function(t)), (lambda: (L.vk_set_transfer_function(ctx.handle, None, 0, 0.0, 1.0), []))
    if entry == "vk_set_projection":
        return (lambda: None), (lambda: (L.vk_set_projection(ctx.handle, N.PROJ_MAX), []))
    held = [iso(0.5), iso(0.3)]
    if step == "set":
        return (lambda: None), (lambda: (L.vk_set_isosurface(ctx.handle, C.byref(held[0])), []))
    if step == "change of threshold":
        return (lambda: ctx.set_isosurface(0.5, (0.9, 0.8, 0.7))), (lambda: (L.vk_set_isosurface(ctx.handle, C.byref(held[1])), []))
    return (lambda: ctx.set_isosurface(0.5, (0.9, 0.8, 0.7))), (lambda: (L.vk_set_isosurface(ctx.handle, None), []))


SETTER_MESSAGES = ("re-layout scratch allocation failed: " + OOM, "distance map allocation failed: " + OOM, "vk_set_transfer_function: the table: " + OOM)


@pytest.mark.parametrize("row", rows("setter"))
def test_a_failed_setter_leaves_the_state_and_the_maps_that_were(E, row):
    entry, step, vol, lay = row.what
    ctx, ref = new_ctx(E), new_ctx(E)
    try:
        calls = []
        for c in (ctx, ref):
            upload(E, c, vol, lay)
            prepare, call = _setter(E, c, entry, step)
            prepare()
            calls.append(call)
        start = state(E, ctx)
        sweep(E, row, ctx, calls[0], lambda m: m in SETTER_MESSAGES)
        rc, _ = calls[1]()
        assert rc == VK_OK, last_error(E, ref)
        got = state(E, ctx)
        assert state_differences(got, state(E, ref)) == "", row.id
        assert got != start, "the step changes what the context holds"
    finally:
        ctx.close()
        ref.close()


# ---- passes --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", rows("pass"))
def test_a_failed_pass_leaves_the_context_and_whole_outputs(E, row):
    p, kind, lay, install = row.what
    V = E.V  # noqa: F811
    c = p.case(kind)
    ctx = new_ctx(E)
    try:
        LH.upload(V, ctx, c.vol, kind, lay)
        start = state(E, ctx)
        opened = []

        def before_call():  # without INSTALL the pass runs inside an open frame, behind the frame's render
            if not install:
                opened.append(ctx.frame_begin())
                V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0).record(ctx)

        def after_call(rc):
            if not install:
                ctx.frame_end()
                assert ctx.read_frame(opened[-1]).tobytes() == start[9], "the recorded frame changed"

        fails, final = sweep(E, row, ctx, lambda: p.call(E, ctx, c, install), lambda m: AC.pass_message_ok(p.entry, m, install), before_call, after_call)
        assert p.final(E, c, final) == "", (row.id, c.name)
        for k, msg, outs in fails:
            assert AC.outputs_against(outs, final) == "", (row.id, k, msg)
        assert all(o.untouched() for o in fails[0][2]), "the first allocation fails before anything is written"
        if not install:
            rc, again = p.call(E, ctx, c, False)  # the hook at 0: the same call, the same outputs, the context as it was
            assert rc == VK_OK and AC.outputs_against(again, final) == "" and not any(o.untouched() for o in again)
            assert state_differences(state(E, ctx), start) == ""
            return
        # INSTALL: what a fresh context holds after uploading the restatement's dense output
        dense, out_kind = p.dense(E, c)
        ref = new_ctx(E)
        try:
            LH.upload(V, ref, np.ascontiguousarray(dense), out_kind, lay)
            assert state_differences(state(E, ctx), state(E, ref)) == "", row.id
        finally:
            ref.close()
    finally:
        ctx.close()


# ---- surfaces: what a slot allocates lazily stays allocated, so every k gets a context of its own ----------------------------------------
def sweep_fresh(E, rid, make, call, after_failure, after_success):
    """make() -> a context; call(ctx) -> rc; after_failure(ctx, k, msg) and after_success(ctx) hold what the row promises."""
    n = 0
    for k in range(1, 66):
        ctx = make()
        try:
            arm(ctx, k)
            rc = call(ctx)
            msg = last_error(E, ctx)
            arm(ctx, 0)
            if rc == VK_OK:
                after_success(ctx)
                break
            assert rc == VK_ERR_OOM and msg.endswith(": " + OOM), (rid, k, rc, msg)
            after_failure(ctx, k, msg)
            n += 1
        finally:
            ctx.close()
    else:
        raise AssertionError(f"{rid}: still failing at k = 65")
    E.summary.append(f"{rid}: {n} allocations ({AC.COUNTS[rid]}), {n} failing calls")
    assert 1 <= n <= 64 and n == AC.COUNTS[rid], (rid, n)


def _with_volume(E, slots=1, vol="u8 sparse", lay="PACKED"):
    ctx = new_ctx(E, slots)
    upload(E, ctx, vol, lay)
    return ctx


def _reference(E, fn, **kw):
    ctx = _with_volume(E, **kw)
    try:
        return fn(ctx)
    finally:
        ctx.close()


def test_first_render_counted_with_the_order_on_the_device(E):
    """The step image, the tile-order ring and its pinned staging."""
    N, L = E.N, E.N.lib()
    rid = "vk_render first, counted, the order on the device"

    def make():
        ctx = _with_volume(E)
        ctx.set_param("order_never_inline", 1)
        return ctx

    def render(ctx):
        return L.vk_render(ctx.handle, N.MODE_NAIVE_TRILINEAR, 0, 0, W, H, 1.0, N.RENDER_COUNT)

    def result(ctx):
        N.check(ctx.handle, L.vk_backbuffer_clear(ctx.handle))
        ctx.reset_step_counts()
        N.check(ctx.handle, render(ctx))
        return ctx.read_backbuffer().tobytes(), ctx.read_steps().tobytes(), ctx.step_counts()

    ref = make()
    try:
        want = result(ref)
        assert want[2][0] > 0
    finally:
        ref.close()
    seen = []

    def after_failure(ctx, k, msg):
        seen.append(msg)
        assert result(ctx) == want  # the next render allocates what is missing and gives the frame

    sweep_fresh(E, rid, make, render, after_failure, lambda ctx: None)
    assert seen == ["render: the step image: " + OOM, "render: the tile-order ring: " + OOM, "render: the tile-order ring's pinned staging: " + OOM]


def test_first_geometry_pass(E):
    L = E.N.lib()
    rid = "vk_render_geometry first"

    def make():
        ctx = _with_volume(E)
        ctx.set_isosurface(0.5)
        return ctx

    def geometry(ctx):
        return L.vk_render_geometry(ctx.handle, 0, 0, W, H, 1.0, 0)

    def result(ctx):
        E.N.check(ctx.handle, geometry(ctx))
        return tuple(a.tobytes() for a in ctx.read_geometry())

    ref = make()
    try:
        want = result(ref)
    finally:
        ref.close()

    def after_failure(ctx, k, msg):
        assert msg == "vk_render_geometry: the geometry surface: " + OOM
        assert L.vk_geometry_info(ctx.handle, None, None, None) == VK_ERR_INVALID  # no surface stays behind
        assert result(ctx) == want

    sweep_fresh(E, rid, make, geometry, after_failure, lambda ctx: None)


def test_first_slice_pass_with_values(E):
    V, L = E.V, E.N.lib()  # noqa: F811
    rid = "vk_render_slice first with VK_SLICE_VALUES"
    plane = V.Slice.axial((37, 21, 11), 5, W, H)

    def slice_(ctx):
        return L.vk_render_slice(ctx.handle, C.byref(plane), 0, 0, W, H, V.SLICE_VALUES)

    def result(ctx):
        E.N.check(ctx.handle, slice_(ctx))
        return ctx.read_slice_values().tobytes(), ctx.read_backbuffer().tobytes()

    want = _reference(E, result)

    def after_failure(ctx, k, msg):
        assert msg == "vk_render_slice: the value surface: " + OOM
        assert L.vk_slice_values_info(ctx.handle, None, None, None) == VK_ERR_INVALID  # no surface stays behind
        assert result(ctx) == want

    sweep_fresh(E, rid, lambda: _with_volume(E), slice_, after_failure, lambda ctx: None)


@pytest.mark.parametrize("bgra", (0, 1), ids=("rgba8", "with bgra8"))
def test_first_present(E, bgra):
    L = E.N.lib()
    rid = "vk_present first, with the Bgra8 target" if bgra else "vk_present first"

    def make():
        ctx = _with_volume(E)
        frame_of(E, ctx)
        return ctx

    def result(ctx):
        E.N.check(ctx.handle, L.vk_present(ctx.handle, W, H, bgra))
        return tuple(None if a is None else a.tobytes() for a in ctx.present_targets())

    ref = make()
    try:
        want = result(ref)
        assert (want[1] is not None) == bool(bgra)
    finally:
        ref.close()
    seen = []

    def after_failure(ctx, k, msg):
        seen.append(msg)
        assert L.vk_present_info(ctx.handle, None, None, None, None) == VK_ERR_INVALID  # no target of a failed pair stays behind
        assert result(ctx) == want  # the next present gives the right bytes

    sweep_fresh(E, rid, make, lambda ctx: L.vk_present(ctx.handle, W, H, bgra), after_failure, lambda ctx: None)
    assert seen == ["vk_present: the Rgba8 target: " + OOM, "vk_present: the Bgra8 target: " + OOM][:1 + bgra]


def test_first_batch(E):
    import torch

    V = E.V  # noqa: F811
    rid = "vk_render_batch first"
    cams = [V.Camera(1.0 + 0.1 * k, 0.5, 1.0, (0.5, 0.5, 0.5), W / H).get_proj_view_matrix() for k in range(2)]
    pipe = V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=1.0)
    out = torch.zeros(len(cams) * H * W * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    blob = b"".join(cams)

    def batch(ctx):
        bid, act = C.c_uint32(), C.c_uint32()
        return E.N.lib().vk_render_batch(ctx.handle, pipe.mode, len(cams), blob, 64, 0, 1, pipe.dt_scale, pipe.flags, C.c_void_p(out.data_ptr()), 0, 0, C.byref(bid), C.byref(act))

    def result(ctx):
        out.zero_()
        torch.cuda.synchronize()
        E.N.check(ctx.handle, batch(ctx))
        ctx.sync()
        return out.cpu().numpy().tobytes()

    want = _reference(E, result)
    assert any(want)
    seen = []

    def after_failure(ctx, k, msg):
        seen.append(msg)
        assert result(ctx) == want

    sweep_fresh(E, rid, lambda: _with_volume(E), batch, after_failure, lambda ctx: None)
    assert seen == ["vk_render_batch: the batch tables: " + OOM, "vk_render_batch: the batch tables' pinned staging: " + OOM]


@pytest.mark.parametrize("slots", (1, 3), ids=("one slot", "three slots"))
def test_backbuffer_resize(E, slots):
    """A failed resize leaves no backbuffer in any slot: render, present and frame begin refuse with their "no backbuffer" messages until a
    resize succeeds; one to the old shape then gives the old frame."""
    N, L = E.N, E.N.lib()
    rid = "vk_backbuffer_resize, " + ("one slot" if slots == 1 else "three slots")
    want = _reference(E, lambda ctx: frame_of(E, ctx), slots=slots)

    def make():
        ctx = _with_volume(E, slots)
        assert frame_of(E, ctx) == want
        return ctx

    def resize(ctx):
        return L.vk_backbuffer_resize(ctx.handle, 96, 80, N.OUT_RGBA32F)

    def after_failure(ctx, k, msg):
        assert msg == "vk_backbuffer_resize: the backbuffer: " + OOM
        w, h = C.c_uint32(7), C.c_uint32(7)
        p = C.c_void_p(0x1234)
        assert L.vk_backbuffer_info(ctx.handle, C.byref(w), C.byref(h), None, C.byref(p)) == VK_OK and (w.value, h.value, p.value) == (0, 0, None)
        fid = C.c_uint64()
        for refused, text in ((lambda: L.vk_render(ctx.handle, N.MODE_NAIVE_TRILINEAR, 0, 0, W, H, 1.0, 0), "render: no backbuffer (vk_backbuffer_resize)"),
                              (lambda: L.vk_present(ctx.handle, W, H, 0), "vk_present: no backbuffer"),
                              (lambda: L.vk_frame_begin(ctx.handle, C.byref(fid)), "vk_frame_begin: no backbuffer (vk_backbuffer_resize)")):
            assert (refused(), last_error(E, ctx)) == (VK_ERR_INVALID, text)
        assert L.vk_backbuffer_resize(ctx.handle, W, H, N.OUT_RGBA32F) == VK_OK, last_error(E, ctx)
        assert frame_of(E, ctx) == want
        for _ in range(slots + 1):  # every slot of the ring has its surface again
            f = ctx.frame_begin()
            N.check(ctx.handle, L.vk_render(ctx.handle, N.MODE_NAIVE_TRILINEAR, 0, 0, W, H, 1.0, 0))
            ctx.frame_end()
            assert ctx.read_frame(f).tobytes() == want
        assert resize(ctx) == VK_OK, last_error(E, ctx)  # ... and the resize that failed goes through

    def after_success(ctx):
        w, h = C.c_uint32(), C.c_uint32()
        assert L.vk_backbuffer_info(ctx.handle, C.byref(w), C.byref(h), None, None) == VK_OK and (w.value, h.value) == (96, 80)

    sweep_fresh(E, rid, make, resize, after_failure, after_success)


def test_frames_in_flight_one_to_three(E):
    """A failed ring leaves one slot on the context's own stream, and a render gives the old frame."""
    N, L = E.N, E.N.lib()
    rid = "vk_ctx_frames_in_flight 1 -> 3"
    want = _reference(E, lambda ctx: frame_of(E, ctx))

    def make():
        ctx = _with_volume(E)
        assert frame_of(E, ctx) == want
        return ctx

    def ring(ctx):
        return L.vk_ctx_frames_in_flight(ctx.handle, 3)

    def frames(ctx, n):
        for _ in range(n):
            f = ctx.frame_begin()
            N.check(ctx.handle, L.vk_render(ctx.handle, N.MODE_NAIVE_TRILINEAR, 0, 0, W, H, 1.0, 0))
            ctx.frame_end()
            assert ctx.read_frame(f).tobytes() == want

    def after_failure(ctx, k, msg):
        assert msg == "vk_ctx_frames_in_flight: the backbuffer: " + OOM
        assert L.vk_ctx_set_stream(ctx.handle, None) == VK_OK, last_error(E, ctx)  # refused on a ring of more than one slot
        assert frame_of(E, ctx) == want
        frames(ctx, 2)
        assert ring(ctx) == VK_OK, last_error(E, ctx)
        frames(ctx, 4)

    sweep_fresh(E, rid, make, ring, after_failure, lambda ctx: frames(ctx, 4))


# ---- leaks -----------------------------------------------------------------------------------------------------------------------------------
def _leak_case(p, vol):
    c = p.case("u8")
    over = dict(vol=vol, name=c.name + ", on the leak volume")
    if hasattr(c, "dims"):  # resample: the whole box, to three quarters
        over.update(box=(0, 0, 0) + AC.LEAK_DIMS, dims=tuple(3 * n // 4 for n in AC.LEAK_DIMS))
    if hasattr(c, "iso"):  # the mesh: a threshold the stand-in crosses
        over.update(iso=0.5)
    if getattr(c, "labels", None) is not None:
        over.update(labels=(vol > 127).astype(np.uint32), max_label=1)
    return c._replace(**over)


LEAK_ROWS = [pytest.param(p, id=p.name) for p in AC.PASSES] + [pytest.param(None, id="vk_volume_upload PACKED")]


@pytest.mark.parametrize("p", LEAK_ROWS)
def test_failing_calls_lose_no_device_memory(E, p):
    """40 failing calls at every k of a pass (with INSTALL where it has the flag, so that the build's allocations are among them) and of the
    PACKED build, on a u8 PACKED volume of 128 x 64 x 32 whose per-voxel u32 arrays are 1 MiB each: less than 8 MiB lost, the margin of the
    suite's other leak tests.  One leaked per-voxel buffer per call would cost 10 MiB or more at any k.  A leak of a fixed-size buffer of a
    few bytes does not show this way: those stand on the RAII types (DeviceTemp, VolBuild, DenseSource, CellScratch, PairScratch) that
    DESIGN.md section 23.1 names per exit."""
    import torch

    V, L = E.V, E.N.lib()  # noqa: F811
    vol = E.expected(("volume", "leak"), lambda: V.volumes.bonsai_standin(AC.LEAK_DIMS))
    assert vol.size == 256 * 1024

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    ctx = new_ctx(E)
    try:
        LH.upload(V, ctx, vol, "u8", "PACKED")
        if p is None:
            call = lambda: L.vk_volume_upload(ctx.handle, vol.ctypes.data, None, AC.LEAK_DIMS[0], AC.LEAK_DIMS[1], AC.LEAK_DIMS[2], E.N.FMT_R8_UNORM, E.N.LAYOUT_PACKED)  # noqa: E731
            n = 8
        else:
            c = _leak_case(p, vol)
            call = lambda: p.call(E, ctx, c, p.install)[0]  # noqa: E731
            n = AC.COUNTS[f"{p.name}{', INSTALL' if p.install else ''}, u8 PACKED"]

        def failing(k):
            arm(ctx, k)
            rc = call()
            arm(ctx, 0)
            assert rc == VK_ERR_OOM, (k, rc, last_error(E, ctx))

        for k in range(1, n + 1):
            failing(k)
        before = free_bytes()
        made = 0
        for k in range(1, n + 1):
            for _ in range(AC.LEAK_CALLS):
                failing(k)
                made += 1
        lost = before - free_bytes()
        E.summary.append(f"leak, {p.name if p else 'vk_volume_upload PACKED'}: {n} allocations, {made} failing calls, {lost / 2**20:.2f} MiB lost")
        assert made == AC.LEAK_CALLS * n and lost < AC.LEAK_MARGIN, f"{lost / 2**20:.1f} MiB of device memory lost over {made} failing calls"
    finally:
        ctx.close()
