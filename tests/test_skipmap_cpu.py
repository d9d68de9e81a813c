"""The skip maps' reference (tests/np_skipmap_reference.py) and case list (tests/skipmap_cases.py) held to themselves, without a GPU, so
that tests/test_skipmap_gpu.py compares the library's bytes with something that is right and cannot pass vacuously.

  the transform    on random small grids the shell-by-shell shifted minima agree with the definition evaluated cell by cell, for the
                   isotropic map and the eight octants, below and at saturation; both invariants hold for its output, and each fails for a
                   byte that is one too large or one too small
  the grid         cell_index is the inverse of the decomposition pack_cells_kernel makes of a storage index; the tap gather agrees with
                   np_u16_reference.cell_taps
  the seed         the empty share equals np_u16_reference.empty_fraction on the u16 cases, and the shares the MAX and isosurface case
                   lists are built for (mip_cases / iso_cases: empty = 0.0 and 1.0)
  the codes        the ctypes shim around vk_tf.hpp's speckle_code builds with plain g++ and agrees with an integer restatement (its
                   sanitizer coverage is tests/speckle_fuzz.cpp's)
  the list         the conditions below"""
import itertools

import numpy as np
import pytest

import iso_cases
import mip_cases
import np_skipmap_reference as SK
import np_u16_reference as NU
import skipmap_cases as SC


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return SK.build_speckle_shim(tmp_path_factory.mktemp("skipmap_shim"))


@pytest.fixture(scope="module")
def referenced(shim):
    """(case, state name) -> (grid, maps, nonempty, share)."""
    return {(c.name, s): SK.reference_maps(c.vol, SC.state_of(c, s), shim) for c in SC.cases() for s in c.states}


OCTANTS = [None] + list(range(8))


def test_transform_is_the_definition():
    rng = np.random.default_rng(5)
    n = 0
    for shape, R in (((5, 4, 6), 2), ((3, 9, 2), 3), ((1, 1, 30), 24), ((2, 28, 1), 24), ((6, 6, 6), 24), ((4, 3, 5), 1)):
        for p in (0.0, 0.01, 0.05, 0.3, 1.0):
            ne = rng.random(shape) < p
            if p == 0.01:
                ne[:] = False
                ne[tuple(int(rng.integers(0, s)) for s in shape)] = True  # a single cell
            for o in OCTANTS:
                got, want = SK.transform(ne, R, o), SK.transform_loop(ne, R, o)
                assert (got == want).all(), (shape, R, p, o)
                assert SK.safe(got, ne, R, o).all() and SK.tight(got, ne, R, o).all(), (shape, R, p, o)
                n += 1
    assert n == 6 * 5 * 9


def test_the_invariants_tell_a_long_byte_from_a_short_one():
    rng = np.random.default_rng(6)
    ne = rng.random((4, 7, 9)) < 0.04
    for o in OCTANTS:
        d = SK.transform(ne, 24, o)
        longer = np.where(d < 25, d + 1, d).astype(np.uint8)
        shorter = np.where(d > 0, d - 1, d).astype(np.uint8)
        assert (SK.safe(longer, ne, 24, o) == (d == 25)).all()       # one too large: unsafe wherever the byte moved
        assert SK.safe(shorter, ne, 24, o).all()
        assert (SK.tight(shorter, ne, 24, o) == (d == 0)).all()      # one too small: not tight wherever the byte moved
        coded = np.where(d == 0, 0x9F, d).astype(np.uint8)           # a code stands for the 0 it replaces
        assert SK.safe(coded, ne, 24, o).all() and SK.tight(coded, ne, 24, o).all()


def test_cell_index_inverts_the_storage_order():
    for nbx, nby, nbz in ((2, 2, 2), (3, 2, 5), (7, 1 + 1, 3), (30, 3, 3)):
        ids = np.arange(nbx * nby * nbz * 64)
        brick, w = ids >> 6, ids & 63
        bx, rest = brick % nbx, brick // nbx
        by, bz = rest % nby, rest // nby
        x, y, z = bx * 4 + (w & 3), by * 4 + ((w >> 2) & 3), bz * 4 + (w >> 4)
        assert (SK.cell_index(x, y, z, nbx, nby) == ids).all()
        stored = (ids % 251).astype(np.uint8)
        grid = (4 * nbx, 4 * nby, 4 * nbz)
        assert (SK.unbrick(stored, grid)[z, y, x] == stored).all()


def test_tap_gather_and_seed_agree_with_the_u16_census():
    n = 0
    for c in SC.cases():
        if c.fmt != "u16":
            continue
        for a, b in zip(SK.cell_taps(c.vol), NU.cell_taps(c.vol)):
            assert a.shape == b.shape and (a == b).all(), c
        for s in c.states:
            st = SC.state_of(c, s) or {}
            want = NU.empty_fraction(c.vol, table=st.get("table"), domain=st.get("domain", (0.0, 1.0)), mip=bool(st.get("mip")), iso=st.get("iso"))
            e = SK.seed_empty(c.vol, st)
            assert float(e.sum()) / e.size == want, (c, s)
            n += 1
    assert n >= 100


def test_seed_counts_the_shares_the_max_and_iso_lists_are_built_for(O):
    n = 0
    for c in mip_cases.cases(O):
        if c.empty is not None:
            e = SK.seed_empty(c.vol, {"mip": True, "table": c.table, "domain": c.domain})
            assert float(e.sum()) / e.size == c.empty, c
            n += 1
    for c in iso_cases.cases(O):
        if c.empty is not None:
            e = SK.seed_empty(c.vol, {"iso": c.iso})
            assert float(e.sum()) / e.size == c.empty, c
            n += 1
    assert n >= 8


def test_speckle_shim_builds_and_agrees_with_integers(shim):
    rng = np.random.default_rng(9)
    vol = rng.integers(0, 26, (14, 15, 16)).astype(np.uint8)
    vol[rng.random(vol.shape) < 0.01] = 255
    vol[rng.random(vol.shape) < 0.01] = 26
    vol[rng.random(vol.shape) < 0.01] = 60
    got = SK.speckle_codes(shim, vol)
    t = np.stack(SK.cell_taps(vol)).astype(np.int64)        # [8, gz, gy, gx]
    hot = t > 25
    lone = hot.sum(axis=0) == 1
    which = hot.argmax(axis=0)
    v = t.max(axis=0)
    m = np.where(hot, 0, t).max(axis=0)
    q = np.where(lone, (16 * (25 - m)) // np.maximum(v - m, 1), 0)
    want = np.where(lone & (q >= 1), 0x80 | (which << 4) | q, 0)
    assert (got == want).all() and (got != 0).sum() > 100 and len(np.unique(got >> 4)) == 9  # every corner, and none


def test_case_list_conditions(referenced):
    cases = SC.cases()
    by_name = {c.name: c for c in cases}
    assert len(by_name) == len(cases)
    assert max(c.vol.size for c in cases) <= 80_000 and sum(c.vol.size <= 40_000 for c in cases) >= len(cases) - 2  # (the speckle volume: 63 360)
    total = 0
    families = {}
    for (name, s), (grid, maps, ne, share) in referenced.items():
        c = by_name[name]
        total += maps.size
        assert maps.shape[0] == (8 if share >= 0.30 else 1) and maps.shape[1:] == grid[::-1]
        assert grid == tuple(4 * (((n - 1) >> 2) + 2) for n in c.dims)
        if maps.shape[0] == 8 and ne.any():   # (an empty volume's eight maps are all 25)
            for a, b in itertools.combinations(range(8), 2):
                assert (maps[a] != maps[b]).any(), (name, s, a, b)
        if not (c.fmt == "u8" and s == "builtin"):
            assert maps.max() <= 25, (name, s)
        if c.kind == "share":
            side = "on" if c.tags[0] == SC.SHARE_EMPTY else ("under" if c.tags[0] < SC.SHARE_EMPTY else "over")
            assert int((~ne).sum()) == c.tags[0] and ne.size == 1280, (name, s)
            assert maps.shape[0] == (1 if side == "under" else 8)
            families.setdefault(SC.family_of(s), set()).add(side)
    # every long blob case: distances beyond what a 48-voxel fuzz volume holds, the last distance of the window and its saturation
    n_long = 0
    for c in cases:
        if c.kind == "long" and c.tags[1] not in ("empty", "full"):
            plain = SK.plain(referenced[c.name, "builtin"][1])
            assert referenced[c.name, "builtin"][1].shape[0] == 8
            assert (plain == 24).any() and (plain == 25).any() and ((plain >= 14) & (plain < 24)).any(), c
            n_long += 1
        if c.kind == "long" and c.tags[1] == "empty":
            assert (referenced[c.name, "builtin"][1] == 25).all() and referenced[c.name, "builtin"][1].shape[0] == 8
        if c.kind == "long" and c.tags[1] == "full":
            assert (SK.plain(referenced[c.name, "builtin"][1]) == 0).all() and referenced[c.name, "builtin"][1].shape[0] == 1
    assert n_long == 3 * 5 * 3
    # the windows of two blobs meet, touch and miss: between blobs 49, 50 and 51 cells apart the isotropic distance would reach 24, 25 on
    # one cell and 25 on two; in the octant maps that is the +x map's last 24 meeting the -x map's
    for axis, a in (("x", 2), ("y", 1), ("z", 0)):
        for apart in (49, 50, 51):
            maps = referenced[f"long {axis} apart {apart} u8", "builtin"][1]
            up, down = SK.plain(maps[1 << (2 - a)]), SK.plain(maps[0])
            line = [slice(5, 6)] * 3          # a row of cells through the blobs (low-corner voxel 1 on the short axes)
            line[a] = slice(None)
            both = np.minimum(up[tuple(line)], down[tuple(line)]).ravel()
            between = both[16:15 + apart]    # the blobs' non-empty cells: 13 .. 15 and 15 + apart .. 17 + apart
            assert int((between == 25).sum()) == {49: 0, 50: 1, 51: 2}[apart], (axis, apart, between)
    # the isotropic map reaches its saturation too
    iso_gap = referenced["gap u8", "builtin"][1]
    assert iso_gap.shape[0] == 1 and (SK.plain(iso_gap) == 25).any() and (SK.plain(iso_gap) == 24).any()
    # all four predicates of the seed on both sides of the 30 % decision and exactly on it
    assert families == {f: {"under", "on", "over"} for f in ("built-in", "table", "max", "iso")}, families
    # the codes: enough of them, and some where the volume ends
    for c in cases:
        if "codes" in c.tags:
            grid, maps, ne, share = referenced[c.name, "builtin"]
            coded = maps[0] >= 128
            for m in maps[1:]:
                assert ((m >= 128) == coded).all()
            if c.name == "speckle volume, all 255":
                continue  # (its hot voxels are too hot to code; the blob's rim and the adjacent pair are not)
            assert coded.sum() >= 20, (c, int(coded.sum()))
            z, y, x = np.nonzero(coded)
            nx, ny, nz = c.dims
            on_face = (x == 4) | (x == nx + 2) | (y == 4) | (y == ny + 2) | (z == 4) | (z == nz + 2)  # low-corner voxel 0 or n - 2
            assert on_face.any(), c
    assert {c.name for c in cases if "codes" in c.tags} == {"speckle volume", "speckle volume, all 255"}
    assert total >= SC.MIN_TOTAL_CELLS, total
    # more than 4 bricks on every axis, in turn
    assert {tuple(g > 16 for g in referenced[c.name, c.states[0]][0]) for c in cases} >= {(True, False, False), (False, True, False), (False, False, True), (True, True, True)}


def test_record_cases(shim):
    for rc in SC.record_cases():
        empty = SK.record_empty(rc.den, rc.nrm)
        assert empty.shape == SK.record_grid(rc.dims)[::-1]
        d = SK.transform(~empty, SK.R_PAIR)
        assert SK.safe(d, ~empty, SK.R_PAIR).all() and SK.tight(d, ~empty, SK.R_PAIR).all()
        assert (~empty).sum() >= 9 and empty.sum() > (~empty).sum()
        nz, ny, nx = rc.den.shape[:3]
        assert empty[0, 1, 5] and empty[0, 2, 6] and not empty[0, 0, 0] and not empty[3, 0, 8]  # NaN and negative opacity; faint ones
        if nx > 100:
            assert d.max() == 61 and (d == 60).any()
            assert not empty[3, 3, 12] and not empty[2, 0, 20] and empty[1, 1, 30] and empty[1, 2, 31]
