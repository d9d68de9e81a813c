"""An independent statement of the skip maps (vk_volume_kernels.hpp: pack_cells_kernel / cell_occ_kernel, dist_pass_kernel and the
lone-speckle codes; vk_volume.hip: build_skip_maps), in numpy: what every byte vk_debug_read_skip_maps returns has to be.

The cell grid.  A PACKED volume of n voxels on an axis stores nb = ((n - 1) >> 2) + 2 bricks of 4 cells there.  The cell at grid
coordinate c has its low-corner voxel at i = c - 4; its two taps on that axis are the voxels clamp(i) and clamp(i + 1), so the first
brick and the end of the last hold padding cells that repeat the volume's faces.  Tap b = dx | dy << 1 | dz << 2.  Arrays of cells are
[gz, gy, gx] here, like the volumes.

The seed.  A cell is non-empty unless the predicate of the state in force calls it empty: the built-in transfer's
(np_builtin_reference.cell_empty; R16_UNORM under np_u16_reference.u16()), a table's (table_cells_empty below: the lookup range of the
cell's taps with one guard entry on each side holds no alpha but 0, np_u16_reference.empty_fraction's form with the finiteness test every
predicate has), the maximum projection's (np_mip_reference.cells_empty) or the isosurface's (np_iso_reference.cells_empty).

The transform.  For octant o = ux | uy << 1 | uz << 2 the byte of cell c is min(d, R + 1), d = min over non-empty q of max |q - c| with q
restricted per axis to q >= c (u = 1) or q <= c (u = 0) and to |q - c| <= R, both sides for the isotropic map; nothing outside the grid
is non-empty.  transform() states it as shifted-array minima, one shell at a time: the L-infinity ball of radius k is the k-fold sum of
the unit cube {-1, 0, 1}^3 (one-sided: {0, u}^3), so the cells within k of a non-empty one are those within 1 of a cell within k - 1 --
26 (7) shifted copies of the reached set per shell, and a cell's byte is the shell that first reaches it.  Nothing here is a separable
pass over one axis.  transform_loop() is the definition as a Python loop per cell; tests/test_skipmap_cpu.py holds the two together.

The codes.  Under the built-in transfer a u8 cell whose lone-speckle code (vk_tf.hpp: speckle_code) is not 0 holds the code, >= 128, in
place of its distance 0.  The code's VALUE is tests/test_speckle_fuzz_cpu.py's business and is taken here from a host build of vk_tf.hpp
(tests/skipmap_speckle_shim.cpp); what the skip-map tests check is its POSITION: which cells carry one, in which states, at which index.

Two invariants, computed by counting non-empty cells in boxes (a summed-area table), not from the transform: `safe` -- the box strictly
within the byte's distance of the cell, on the octant's side, holds no non-empty cell -- and `tight` -- the byte is R + 1 or the box of
its own radius holds one.  A byte that is safe and tight equals the transform; a mismatch names its kind through them.

The records (RGBA16F_PAIR, PACKED): one isotropic map, R = 60, over the grid of 4 ceil(n / 4) records per axis, whose zero set is the
records that can contribute.  np_compute_reference.py has no such predicate; record_empty() restates the one in pack_pairs_kernel's
comment (vk_pair.hpp): the opacity smoothstep(0, 0.7, a^3) is exactly 0, the colour is finite and no normal component is -inf."""
from __future__ import annotations

import ctypes as C
import itertools
import os
import subprocess

import numpy as np

import np_builtin_reference as NB
import np_compute_reference as NC
import np_iso_reference as NI
import np_mip_reference as NM
import np_table_reference as NT
import np_u16_reference as NU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
R_CELLS = 24   # kDistRadius
R_PAIR = 60    # kPairDistRadius
OCTANT_SHARE = 0.30  # build_skip_maps: eight one-sided maps from this share of empty cells on


# ---- the grid ----

def bricks(n):
    return ((n - 1) >> 2) + 2


def grid_of(dims):
    """Cells per axis (gx, gy, gz) of a PACKED volume of dims = (nx, ny, nz)."""
    return tuple(4 * bricks(n) for n in dims)


def fmt_of(vol):
    return {np.dtype(np.uint8): "u8", np.dtype(np.float16): "f16", np.dtype(np.uint16): "u16"}[vol.dtype]


def cell_taps(vol):
    """The eight taps (f32 on the kernel's scale: u8 0..255, u16 0..65535, f16 the value) of every stored cell: [gz, gy, gx] each."""
    nz, ny, nx = vol.shape
    lo, hi = [], []
    for n in (nx, ny, nz):
        i = np.arange(4 * bricks(n)) - 4       # the low-corner voxel of grid coordinate c
        lo.append(np.clip(i, 0, n - 1))
        hi.append(np.clip(i + 1, 0, n - 1))
    pick = (lo, hi)
    return [vol[np.ix_(pick[b >> 2][2], pick[(b >> 1) & 1][1], pick[b & 1][0])].astype(np.float32) for b in range(8)]


def cell_index(x, y, z, nbx, nby):
    """The storage index of cell (x, y, z): bricks x-fastest, 64 cells per brick, x-fastest inside."""
    x, y, z = (np.asarray(v, np.int64) for v in (x, y, z))
    brick = ((z // 4) * nby + (y // 4)) * nbx + (x // 4)
    return brick * 64 + (z % 4) * 16 + (y % 4) * 4 + (x % 4)


def unbrick(stored, grid):
    """A stored map (bricked order, one byte per cell) as [gz, gy, gx]."""
    gx, gy, gz = grid
    if grid not in _STORAGE_INDEX:
        z, y, x = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
        _STORAGE_INDEX[grid] = cell_index(x, y, z, gx // 4, gy // 4)
    return np.asarray(stored)[_STORAGE_INDEX[grid]]


_STORAGE_INDEX = {}


# ---- the seed ----

def table_cells_empty(taps, table, k1, k2):
    """A table's predicate: every tap finite, and entries max(floor(u(m)) - 1, 0) .. min(floor(u(M)) + 2, n - 1) all have alpha 0, m and M
    the cell's smallest and largest tap, u = min(max(fma(t, k1, k2), 0), n - 1)."""
    t = np.stack([np.asarray(v, np.float32) for v in taps])
    finite = np.isfinite(t).all(axis=0)
    safe = np.where(np.isfinite(t), t, f32(0.0))
    m, M = safe.min(axis=0), safe.max(axis=0)
    T = np.ascontiguousarray(table, np.float32)
    n = len(T)
    prefix = np.concatenate([[0], np.cumsum(T[:, 3] != 0)])
    lo = np.maximum(np.floor(NM.tf_u(m, k1, k2, f32(n - 1))).astype(np.int64) - 1, 0)
    hi = np.minimum(np.floor(NM.tf_u(M, k1, k2, f32(n - 1))).astype(np.int64) + 2, n - 1)
    return finite & (prefix[hi + 1] == prefix[lo])


def seed_empty(vol, state=None):
    """The cells [gz, gy, gx] the state in force calls empty.  state: None (the built-in transfer) or a dict with "iso" (the threshold in
    sample values; replaces everything else), "mip" (True: the maximum projection) and "table" / "domain" (None: no table; under "mip"
    the grey ramp)."""
    state = state or {}
    fmt = fmt_of(vol)
    taps = cell_taps(vol)
    table, domain = state.get("table"), state.get("domain", (0.0, 1.0))
    constants = NU.tf_constants if fmt == "u16" else NT.tf_constants
    if state.get("iso") is not None:
        return NI.cells_empty(taps, NU.iso_k(state["iso"]) if fmt == "u16" else NI.iso_k(state["iso"], fmt == "u8"))
    if state.get("mip"):
        n = 2 if table is None else len(table)
        k1, k2 = constants(n, *((0.0, 1.0) if table is None else domain), fmt == "u8")
        return NM.cells_empty(taps, k1, k2, f32(n - 1))
    if table is not None:
        k1, k2 = constants(len(table), domain[0], domain[1], fmt == "u8")
        return table_cells_empty(taps, table, k1, k2)
    if fmt == "u16":
        with NU.u16():
            return NB.cell_empty(taps, False)
    return NB.cell_empty(taps, fmt == "f16")


def is_builtin(state):
    state = state or {}
    return state.get("iso") is None and not state.get("mip") and state.get("table") is None


# ---- the transform ----

def _offsets(octant):
    if octant is None:
        side = [(-1, 0, 1)] * 3
    else:
        side = [(0, 1) if (octant >> a) & 1 else (-1, 0) for a in range(3)]  # x, y, z
    return [(dz, dy, dx) for dz in side[2] for dy in side[1] for dx in side[0] if (dz, dy, dx) != (0, 0, 0)]


def _shifted(a, off):
    """b[c] = a[c + off], False where c + off lies outside the grid."""
    out = np.zeros_like(a)
    src, dst = [], []
    for o, n in zip(off, a.shape):
        if abs(o) >= n:
            return out
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n + min(-o, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def transform(nonempty, R, octant=None):
    """The map [gz, gy, gx] uint8 of octant `octant` (None: the isotropic map) over the seed `nonempty`."""
    reached = np.asarray(nonempty, bool).copy()
    d = np.where(reached, 0, R + 1).astype(np.uint8)
    offs = _offsets(octant)
    for k in range(1, R + 1):
        grown = reached.copy()
        for off in offs:
            grown |= _shifted(reached, off)
        new = grown & ~reached
        if not new.any():
            break
        d[new] = k
        reached = grown
    return d


def transform_loop(nonempty, R, octant=None):
    """The definition, cell by cell and candidate by candidate (small grids only)."""
    ne = np.asarray(nonempty, bool)
    qs = np.argwhere(ne)
    d = np.full(ne.shape, R + 1, np.uint8)
    for c in itertools.product(*(range(n) for n in ne.shape)):
        best = R + 1
        for q in qs:
            dist, ok = 0, True
            for a in range(3):                  # a: z, y, x; the octant's bit of that axis is 2 - a
                j = int(q[a]) - c[a]
                if octant is not None and (j < 0 if (octant >> (2 - a)) & 1 else j > 0):
                    ok = False
                dist = max(dist, abs(j))
            if ok and dist <= R:
                best = min(best, dist)
        d[c] = best
    return d


def _box_counts(nonempty, radius, octant):
    """Per cell: the number of non-empty cells q with |q - c| <= radius[c] per axis on the octant's side (radius < 0: none)."""
    ne = np.asarray(nonempty, bool)
    S = np.zeros(tuple(n + 1 for n in ne.shape), np.int64)
    S[1:, 1:, 1:] = ne.cumsum(0).cumsum(1).cumsum(2)
    r = np.asarray(radius, np.int64)
    idx = np.meshgrid(*(np.arange(n) for n in ne.shape), indexing="ij")
    lo, hi = [], []
    for a in range(3):
        up = octant is None or bool((octant >> (2 - a)) & 1)
        down = octant is None or not (octant >> (2 - a)) & 1
        lo.append(np.maximum(idx[a] - (r if down else 0), 0))
        hi.append(np.minimum(idx[a] + (r if up else 0), ne.shape[a] - 1) + 1)
    total = np.zeros(ne.shape, np.int64)
    for cz, cy, cx in itertools.product((0, 1), repeat=3):
        sign = (-1) ** (3 - cz - cy - cx)
        total += sign * S[(hi if cz else lo)[0], (hi if cy else lo)[1], (hi if cx else lo)[2]]
    return np.where(r >= 0, total, 0)


def plain(byte_map):
    """A map with its codes read as the distance 0 they stand for."""
    m = np.asarray(byte_map)
    return np.where(m >= 128, 0, m).astype(np.int64)


def safe(byte_map, nonempty, R, octant=None):
    """Per cell: no non-empty cell lies strictly within the byte's distance (on the octant's side)."""
    return _box_counts(nonempty, plain(byte_map) - 1, octant) == 0


def tight(byte_map, nonempty, R, octant=None):
    """Per cell: the byte is as large as it may be -- R + 1, or a non-empty cell lies at its distance."""
    m = plain(byte_map)
    return (m == R + 1) | ((m <= R) & (_box_counts(nonempty, np.minimum(m, R), octant) > 0))


# ---- the codes ----

def build_speckle_shim(out_dir):
    """tests/skipmap_speckle_shim.cpp (vk_tf.hpp's speckle_code behind a C entry point), plain g++; returns the loaded CDLL."""
    so = os.path.join(str(out_dir), "libskipmap_speckle_shim.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "vokselis_amd", "csrc"),
                    "-o", so, os.path.join(ROOT, "tests", "skipmap_speckle_shim.cpp")], check=True)
    L = C.CDLL(so)
    L.skm_speckle_codes.restype = None
    L.skm_speckle_codes.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    return L


def speckle_codes(shim, vol):
    """The lone-speckle code (0: none) of every stored cell of a u8 volume: [gz, gy, gx] uint8."""
    assert vol.dtype == np.uint8
    taps = np.ascontiguousarray(np.stack(cell_taps(vol), axis=-1), np.float32)  # [gz, gy, gx, 8]
    out = np.zeros(taps.shape[:3], np.uint8)
    shim.skm_speckle_codes(taps.ctypes.data, out.size, out.ctypes.data)
    return out


# ---- the maps of a volume in a state ----

_TRANSFORMED = {}


def reference_maps(vol, state=None, shim=None):
    """(grid, maps [n_maps, gz, gy, gx] uint8, nonempty [gz, gy, gx], empty share) of a PACKED / PACKED_PAIRS volume in `state`.  shim: the
    loaded speckle shim; needed for u8 volumes under the built-in transfer."""
    empty = seed_empty(vol, state)
    ne = ~empty
    share = float(empty.sum()) / float(empty.size)
    octants = list(range(8)) if share >= OCTANT_SHARE else [None]
    key = (ne.shape, ne.tobytes(), len(octants))  # many (volume, state) pairs share a seed: each is transformed once
    if key not in _TRANSFORMED:
        _TRANSFORMED[key] = np.stack([transform(ne, R_CELLS, o) for o in octants])
    maps = _TRANSFORMED[key]
    if vol.dtype == np.uint8 and is_builtin(state):
        code = speckle_codes(shim, vol)
        assert not (empty & (code != 0)).any()  # (a coded cell has a tap above 25)
        maps = np.where(code[None] != 0, code[None], maps)
    nz, ny, nx = vol.shape
    return grid_of((nx, ny, nz)), maps, ne, share


# ---- the records ----

def record_grid(dims):
    return tuple(4 * ((n + 3) // 4) for n in dims)


def record_empty(den, nrm):
    """The records [gz, gy, gx] that cannot contribute (vk_pair.hpp, restated): opacity exactly 0, finite colour, no -inf normal
    component.  den, nrm: f16 [nz, ny, nx, 4]; the records beyond the volume are zeros, which are empty."""
    nz, ny, nx = den.shape[:3]
    gx, gy, gz = record_grid((nx, ny, nz))
    d = np.zeros((gz, gy, gx, 4), np.float32)
    n = np.zeros((gz, gy, gx, 4), np.float32)
    d[:nz, :ny, :nx] = np.asarray(den).view(np.float16).astype(np.float32)
    n[:nz, :ny, :nx] = np.asarray(nrm).view(np.float16).astype(np.float32)
    return (NC.opacity(d[..., 3]) == 0) & np.isfinite(d[..., :3]).all(axis=-1) & (n[..., :3] != -np.inf).all(axis=-1)
