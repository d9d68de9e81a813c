"""The skip maps on the MI355X, byte for byte: what vk_debug_read_skip_maps returns -- the bytes the cell marches read -- against the exact
distance transform of tests/np_skipmap_reference.py, over the volumes and states of tests/skipmap_cases.py (tests/test_skipmap_cpu.py holds
both to their conditions).  Every comparison is bitwise.

A map that is too short renders the same frames, step counts, S_ref and S_sampled as a right one, only slower; nothing else in the suite
reads these bytes.  Here a wrong byte is collected with its case, layout, state, octant and cell, and named: UNSAFE (a non-empty cell lies
within its distance: a rendering bug), SHORT (safe, but not the largest safe value: a performance bug) or a MISPLACED CODE."""
import ctypes as C

import numpy as np
import pytest

import np_skipmap_reference as SK
import skipmap_cases as SC
from gpu_helpers import V  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_INVALID = -1  # VK_ERR_INVALID
LAYOUTS_OF = {"u8": ("PACKED", "PACKED_PAIRS"), "f16": ("PACKED",), "u16": ("PACKED",)}
KINDS = ("long", "gap", "edges", "lopsided", "share", "values")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return SK.build_speckle_shim(tmp_path_factory.mktemp("skipmap_shim"))


@pytest.fixture(scope="module")
def referenced(shim):
    """(case name, state name) -> (grid, maps, nonempty, share): computed once for the module."""
    return {(c.name, s): SK.reference_maps(c.vol, SC.state_of(c, s), shim) for c in SC.cases() for s in c.states}


def _context(V):
    return V.Context(16, 16, backbuffer=(16, 16), out_format=V.OUT_RGBA32F)


def _upload(V, ctx, c, layout):
    V.VolumeTexture(ctx, c.vol, layout=getattr(V, "LAYOUT_" + layout), fmt=V.FMT_R16_UNORM if c.fmt == "u16" else None)


def _set_state(ctx, c, name):
    """From the built-in state to `name`."""
    st = SC.state_of(c, name) or {}
    if st.get("table") is not None:
        ctx.set_transfer_function(st["table"], st["domain"])
    if st.get("mip"):
        ctx.set_projection("max")
    if st.get("iso") is not None:
        ctx.set_isosurface(st["iso"])


def _clear_state(ctx):
    ctx.set_isosurface(None)
    ctx.set_projection(None)
    ctx.set_transfer_function(None)


def _read(ctx):
    """(grid, maps [n_maps, gz, gy, gx]) un-bricked."""
    grid, stored = ctx.read_skip_maps()
    gx, gy, gz = grid
    if stored.shape[0] == 0:
        return grid, stored.reshape(0, gz, gy, gx)
    return grid, np.stack([SK.unbrick(m, grid) for m in stored])


def _mismatches(what, got, ref, nonempty, R=SK.R_CELLS):
    """The bytes of `got` that differ from `ref`, each named by its kind (at most four per map are listed)."""
    out = []
    if got.shape != ref.shape:
        return [f"{what}: {got.shape[0]} maps over {got.shape[1:][::-1]}, want {ref.shape[0]} over {ref.shape[1:][::-1]}"]
    for k in range(ref.shape[0]):
        bad = got[k] != ref[k]
        if not bad.any():
            continue
        octant = k if ref.shape[0] == 8 else None
        safe, tight = SK.safe(got[k], nonempty, R, octant), SK.tight(got[k], nonempty, R, octant)
        code = bad & ((got[k] >= 128) | (ref[k] >= 128))
        kinds = np.where(code, "MISPLACED CODE", np.where(~safe, "UNSAFE", np.where(~tight, "SHORT", "neither unsafe nor short")))
        z, y, x = np.nonzero(bad)
        head = f"{what} octant {octant}: {int(bad.sum())} bytes differ ({int((bad & code).sum())} codes, {int((bad & ~code & ~safe).sum())} unsafe, {int((bad & ~code & safe & ~tight).sum())} short)"
        out.append(head + "; " + ", ".join(f"cell ({x[i]}, {y[i]}, {z[i]}) holds {got[k][z[i], y[i], x[i]]}, want {ref[k][z[i], y[i], x[i]]}: {kinds[z[i], y[i], x[i]]}"
                                           for i in range(min(4, len(z)))))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_every_byte_of_every_map(V, referenced, kind):
    """Upload under the built-in transfer, then each state set from it and cleared again (the rebuilds of vk_set_transfer_function,
    vk_set_projection and vk_set_isosurface): n_maps, the grid and every byte are the reference's; PACKED and PACKED_PAIRS of one u8 volume
    hold identical maps."""
    fails, n_maps, n_bytes = [], 0, {}
    want_maps, want_bytes = 0, {}
    ctx = _context(V)
    try:
        for c in (c for c in SC.cases() if c.kind == kind):
            per_layout = {}
            for lay in LAYOUTS_OF[c.fmt]:
                _clear_state(ctx)
                _upload(V, ctx, c, lay)
                for s in c.states:
                    if s != "builtin":
                        _set_state(ctx, c, s)
                    grid, got = _read(ctx)
                    if s != "builtin":
                        _clear_state(ctx)
                    ref_grid, ref, ne, share = referenced[c.name, s]
                    what = f"{c.name} / {lay} / {s} (empty share {share:.4f})"
                    if grid != ref_grid:
                        fails.append(f"{what}: grid {grid}, want {ref_grid}")
                        continue
                    if got.shape[0] != ref.shape[0]:
                        fails.append(f"{what}: {got.shape[0]} maps, want {ref.shape[0]}")
                        continue
                    fails += _mismatches(what, got, ref, ne)
                    if not (c.fmt == "u8" and s == "builtin") and (got >= 128).any():
                        fails.append(f"{what}: {int((got >= 128).sum())} bytes >= 128 in a state without codes")
                    n_maps += got.shape[0]
                    n_bytes[lay] = n_bytes.get(lay, 0) + got.size
                    want_maps += ref.shape[0]
                    want_bytes[lay] = want_bytes.get(lay, 0) + ref.size
                    per_layout[lay, s] = got
                _clear_state(ctx)
                grid, again = _read(ctx)   # the built-in maps after the last state: the first ones, codes included
                if not (again.shape == per_layout[lay, "builtin"].shape and (again == per_layout[lay, "builtin"]).all()):
                    fails.append(f"{c.name} / {lay}: the built-in maps after the states differ from those of the upload")
            if c.fmt == "u8":
                for s in c.states:
                    a, b = per_layout.get(("PACKED", s)), per_layout.get(("PACKED_PAIRS", s))
                    if a is None or b is None or a.shape != b.shape or (a != b).any():
                        fails.append(f"{c.name} / {s}: PACKED and PACKED_PAIRS hold different maps")
    finally:
        ctx.close()
    print(f"\n{kind}: {n_maps} maps read, bytes compared per layout {n_bytes}")
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    assert n_maps == want_maps and n_bytes == want_bytes and n_maps > 0 and min(n_bytes.values()) > 0
    expect = sum(referenced[c.name, s][1].size * len(LAYOUTS_OF[c.fmt]) for c in SC.cases() if c.kind == kind for s in c.states)
    assert sum(n_bytes.values()) == expect


REBUILD_PAIRS = (("speckle volume", "face patch u8"), ("share 384 of 1280 u8", "(9, 5, 13) u8 blobs"), ("f16 edge values", "f16 thresholds"),
                 ("u16 6553 / 6554", "u16 specials"), ("long x apart 50 u16", "corner u16"))


@pytest.mark.parametrize("first,second", REBUILD_PAIRS)
def test_rebuilds_equal_a_fresh_context(V, referenced, shim, first, second):
    """upload; table; MAX; isosurface; isosurface off; table reset (the table, then the projection); a second upload under a table: after
    each step the maps are those of a fresh context put into that state before its upload, and the reference's."""
    by_name = {c.name: c for c in SC.cases()}
    a, b = by_name[first], by_name[second]
    table = {"table": SC.BAND, "domain": SC.DOMAIN}
    steps = [  # (what the step does to the used context, the volume, the state the maps are then built under)
        ("upload", a, None),
        ("table", a, table),
        ("MAX", a, dict(table, mip=True)),
        ("isosurface", a, dict(table, mip=True, iso=a.iso_in)),
        ("isosurface off", a, dict(table, mip=True)),
        ("table reset", a, {"mip": True}),
        ("projection reset", a, None),
        ("second upload under a table", b, table),
    ]
    fails, n = [], 0
    for lay in LAYOUTS_OF[a.fmt]:
        used = _context(V)
        try:
            seen = {}
            for what, c, st in steps:
                if what in ("upload", "second upload under a table"):
                    if st:
                        used.set_transfer_function(st["table"], st["domain"])
                    _upload(V, used, c, lay)
                elif what == "table":
                    used.set_transfer_function(st["table"], st["domain"])
                elif what == "MAX":
                    used.set_projection("max")
                elif what == "isosurface":
                    used.set_isosurface(st["iso"])
                elif what == "isosurface off":
                    used.set_isosurface(None)
                elif what == "table reset":
                    used.set_transfer_function(None)
                else:
                    used.set_projection(None)
                grid, got = _read(used)
                fresh = _context(V)
                try:
                    if st and st.get("table") is not None:
                        fresh.set_transfer_function(st["table"], st["domain"])
                    if st and st.get("mip"):
                        fresh.set_projection("max")
                    if st and st.get("iso") is not None:
                        fresh.set_isosurface(st["iso"])
                    _upload(V, fresh, c, lay)
                    fgrid, want = _read(fresh)
                finally:
                    fresh.close()
                ref_grid, ref, ne, share = SK.reference_maps(c.vol, st, shim)
                tag = f"{c.name} / {lay} / after '{what}'"
                if grid != fgrid or got.shape != want.shape or (got != want).any():
                    fails.append(f"{tag}: the used context's maps differ from a fresh context's")
                if grid != ref_grid:
                    fails.append(f"{tag}: grid {grid}, want {ref_grid}")
                else:
                    fails += _mismatches(tag, got, ref, ne)
                coded = bool((got >= 128).any())
                if st is not None and coded:
                    fails.append(f"{tag}: bytes >= 128 under a table, MAX or an isosurface")
                seen[what] = got
                n += got.size
            if not (seen["projection reset"].shape == seen["upload"].shape and (seen["projection reset"] == seen["upload"]).all()):
                fails.append(f"{a.name} / {lay}: the maps after the final reset are not those of the upload")
            if a.name == "speckle volume" and not (seen["projection reset"] >= 128).sum() >= 20:
                fails.append(f"{a.name} / {lay}: the codes are not back after the final reset")
            if not (seen["isosurface off"] == seen["MAX"]).all():
                fails.append(f"{a.name} / {lay}: isosurface off does not restore the MAX maps")
        finally:
            used.close()
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    assert n > 0


def test_clip_box_lighting_and_shadows_change_no_byte(V):
    c = {c.name: c for c in SC.cases()}["(33, 20, 7) u8 blobs"]
    for lay in LAYOUTS_OF[c.fmt]:
        ctx = _context(V)
        try:
            _upload(V, ctx, c, lay)
            for s in ("builtin", "band", "iso in"):
                _clear_state(ctx)
                _set_state(ctx, c, s)
                before = ctx.read_skip_maps()
                ctx.set_clip_box((0.1, 0.2, 0.0), (0.7, 0.9, 0.6))
                ctx.set_lighting((0.3, 1.0, 0.2))
                ctx.set_shadows(0.6, 2.0)
                during = ctx.read_skip_maps()
                ctx.set_shadows(None)
                ctx.set_lighting(None)
                ctx.set_clip_box(None)
                after = ctx.read_skip_maps()
                assert before[1].size > 0
                for other in (during, after):
                    assert other[0] == before[0] and other[1].shape == before[1].shape and (other[1] == before[1]).all(), (lay, s)
        finally:
            ctx.close()


def test_layouts_without_maps_report_none(V):
    rng = np.random.default_rng(3)
    u8 = rng.integers(0, 256, (9, 10, 11)).astype(np.uint8)
    f16 = rng.uniform(0.0, 1.0, (9, 10, 11)).astype(np.float16)
    u16 = rng.integers(0, 65536, (9, 10, 11)).astype(np.uint16)
    rc = SC.record_cases()[1]
    n = 0
    ctx = _context(V)
    try:
        for vol, fmt, lays in ((u8, None, ("LINEAR", "BRICKED", "QUADS", "STAGED")), (f16, None, ("LINEAR", "BRICKED", "QUADS", "STAGED")),
                               (u16, V.FMT_R16_UNORM, ("LINEAR",))):
            for lay in lays:
                V.VolumeTexture(ctx, vol, layout=getattr(V, "LAYOUT_" + lay), fmt=fmt)
                grid, maps = ctx.read_skip_maps()
                assert grid == (0, 0, 0) and maps.shape == (0, 0), (lay, grid, maps.shape)
                n += 1
        V.VolumeTexture(ctx, rc.den, rc.nrm, layout=V.LAYOUT_LINEAR)
        grid, maps = ctx.read_skip_maps()
        assert grid == (0, 0, 0) and maps.shape == (0, 0)
        V.VolumeTexture(ctx, u8, layout=V.LAYOUT_PACKED)   # and a layout with maps after one without
        grid, maps = ctx.read_skip_maps()
        assert grid == SK.grid_of((11, 10, 9)) and maps.shape[0] in (1, 8) and maps.shape[1] == grid[0] * grid[1] * grid[2]
    finally:
        ctx.close()
    assert n == 9


def test_refusals(V):
    lib = V.native.lib()
    grid, n_maps, nbytes = (C.c_uint32 * 3)(), C.c_uint32(), C.c_size_t()

    def refused(ctx, rc, needle):
        msg = lib.vk_last_error(ctx.handle).decode()
        assert rc == ERR_INVALID and needle in msg, (rc, msg)

    assert lib.vk_debug_read_skip_maps(None, grid, C.byref(n_maps), C.byref(nbytes), None, 0) == ERR_INVALID
    ctx = _context(V)
    try:
        refused(ctx, lib.vk_debug_read_skip_maps(ctx.handle, grid, C.byref(n_maps), C.byref(nbytes), None, 0), "no volume")
        V.VolumeTexture(ctx, np.zeros((5, 6, 7), np.uint8), layout=V.LAYOUT_PACKED)
        V.native.check(ctx.handle, lib.vk_debug_read_skip_maps(ctx.handle, grid, C.byref(n_maps), C.byref(nbytes), None, 0))
        assert tuple(grid) == (12, 12, 12) and n_maps.value == 8 and nbytes.value == 8 * 12 ** 3
        buf = np.full(nbytes.value + 16, 0xAB, np.uint8)
        refused(ctx, lib.vk_debug_read_skip_maps(ctx.handle, None, C.byref(n_maps), C.byref(nbytes), None, 0), "vk_debug_read_skip_maps")
        refused(ctx, lib.vk_debug_read_skip_maps(ctx.handle, grid, None, C.byref(nbytes), None, 0), "vk_debug_read_skip_maps")
        refused(ctx, lib.vk_debug_read_skip_maps(ctx.handle, grid, C.byref(n_maps), None, None, 0), "vk_debug_read_skip_maps")
        refused(ctx, lib.vk_debug_read_skip_maps(ctx.handle, grid, C.byref(n_maps), C.byref(nbytes), buf.ctypes.data, nbytes.value - 1), "buffer")
        assert (buf == 0xAB).all()  # a refused call writes nothing
        V.native.check(ctx.handle, lib.vk_debug_read_skip_maps(ctx.handle, grid, C.byref(n_maps), C.byref(nbytes), buf.ctypes.data, nbytes.value))
        assert (buf[:nbytes.value] == 25).all() and (buf[nbytes.value:] == 0xAB).all()  # an empty volume, and not a byte beyond
    finally:
        ctx.close()


def test_record_map_is_the_transform_of_its_own_zero_set(V):
    """RGBA16F_PAIR, PACKED: one map over the record grid, embedded in the records.  It is the exact isotropic transform (R = 60) of its
    own zero set -- which needs no predicate -- and that zero set is the records np_skipmap_reference.record_empty calls non-empty, which
    restates vk_pair.hpp rather than verifying it."""
    fails, n = [], 0
    ctx = _context(V)
    try:
        for rc in SC.record_cases():
            V.VolumeTexture(ctx, rc.den, rc.nrm, layout=V.LAYOUT_PACKED)
            grid, got = _read(ctx)
            assert grid == SK.record_grid(rc.dims) and got.shape[0] == 1, (rc.name, grid, got.shape)
            zero = got[0] == 0
            fails += _mismatches(f"{rc.name} against the transform of its own zero set", got, SK.transform(zero, SK.R_PAIR)[None], zero, SK.R_PAIR)
            want = ~SK.record_empty(rc.den, rc.nrm)
            if (zero != want).any():
                z, y, x = np.nonzero(zero != want)
                fails.append(f"{rc.name}: {len(z)} records differ from the predicate, first ({x[0]}, {y[0]}, {z[0]}): map byte {got[0][z[0], y[0], x[0]]}, non-empty {bool(want[z[0], y[0], x[0]])}")
            if rc.dims[0] >= 248 and not (got.max() == 61 and (got == 60).any()):
                fails.append(f"{rc.name}: the map does not reach 60 and its saturation 61 (max {got.max()})")
            n += got.size
    finally:
        ctx.close()
    assert not fails, "\n".join(fails)
    assert n == sum(int(np.prod(SK.record_grid(rc.dims))) for rc in SC.record_cases()) > 0


def test_the_march_reads_these_bytes(V, O, referenced):
    """The anchor: on an octant case whose maps equal the reference, the frame under RENDER_FORCE_SKIP is bitwise the RENDER_NO_SKIP frame
    (asserted elsewhere too; here so that the bytes checked above are seen to be the ones a march walks by)."""
    c = {c.name: c for c in SC.cases()}["speckle volume"]
    W, H = 96, 64
    ctx = V.Context(W, H, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        _upload(V, ctx, c, "PACKED")
        grid, got = _read(ctx)
        ref = referenced[c.name, "builtin"][1]
        assert got.shape[0] == 8 and (got == ref).all()
        ctx.set_camera_blob(O.camera_blob(1.1, 0.45, 0.9, (0.5, 0.5, 0.5), W / H))
        frames = []
        for flags in (V.RENDER_FORCE_SKIP, V.RENDER_NO_SKIP):
            V.native.check(ctx.handle, V.native.lib().vk_backbuffer_clear(ctx.handle))
            V.RaycastPipeline(V.MODE_NAIVE_TRILINEAR, dt_scale=0.5, flags=flags).record(ctx)
            frames.append(ctx.read_backbuffer().copy())
    finally:
        ctx.close()
    assert (frames[0].view(np.uint32) == frames[1].view(np.uint32)).all() and (frames[0][..., :3] > 0).any()
