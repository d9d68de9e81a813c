"""The shared case list of the histogram tests (vk_volume_histogram): small volumes of the three formats -- the odd
dimensions are there for the duplicate taps a cell layout bakes into its last cells -- and for each a set of requests: a voxel box, a bin
count, a domain.  The CPU suite holds the C restatement to the numpy reference over it (tests/test_hist_fuzz_cpu.py), the GPU suite every
layout's kernels to the restatement (tests/test_hist_fuzz_gpu.py).  A volume is shared by its requests (`vol_id`): the GPU driver uploads
it once per layout."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name vol_id kind vol box bins domain")

DIMS = ((1, 1, 1), (5, 3, 2), (17, 9, 6), (24, 24, 24), (33, 20, 7))  # nx, ny, nz
BINS = (1, 2, 255, 256, 1000, 4096)
# domains in sample values: inside, around and beside the data, and the identity's [0, 1]
DOMAINS = {"u8": ((0.2, 0.6), (-0.5, 1.5), (1.5, 2.5), (0.0, 1.0)),
           "u16": ((0.017, 0.02), (-0.25, 1.25), (0.5, 0.9), (0.0, 1.0)),
           "f16": ((0.25, 0.75), (-4.0, 4.0), (10.0, 20.0), (0.0, 1.0))}


def _odd_below(n):
    """The largest odd extent that fits behind origin 1 on an axis of n voxels (at least 1)."""
    e = n - 1
    return max(e - (e % 2 == 0), 1)


def boxes(nx, ny, nz):
    """(name, ((x0, y0, z0), (x1, y1, z1))): the whole volume (None), one voxel, an empty box, odd origins and odd extents, boxes that
    touch each face, the last plane of each axis alone."""
    out = [("whole", None), ("one voxel", ((nx // 2, ny // 2, nz // 2), (nx // 2 + 1, ny // 2 + 1, nz // 2 + 1))),
           ("empty", ((nx // 2, 0, 0), (nx // 2, ny, nz)))]
    if min(nx, ny, nz) >= 2:
        out.append(("odd origin, odd extent", ((1, 1, 1), (1 + _odd_below(nx), 1 + _odd_below(ny), 1 + _odd_below(nz)))))
        out.append(("low faces", ((0, 0, 0), ((nx + 1) // 2, (ny + 1) // 2, (nz + 1) // 2))))
        out.append(("high faces", ((nx // 2, ny // 2, nz // 2), (nx, ny, nz))))
        out.append(("last z plane", ((0, 0, nz - 1), (nx, ny, nz))))
        out.append(("last x plane", ((nx - 1, 0, 0), (nx, ny, nz))))
        out.append(("last y row of an odd origin", ((1, ny - 1, 0), (nx, ny, nz))))
    fixed = []
    for name, b in out:
        if b is not None:
            lo, hi = b
            hi = (min(hi[0], nx), min(hi[1], ny), min(hi[2], nz))
            lo = (min(lo[0], hi[0]), min(lo[1], hi[1]), min(lo[2], hi[2]))
            b = (lo, hi)
        fixed.append((name, b))
    return fixed


def f16_next(x, up):
    return np.nextafter(np.float16(x), np.float16(np.inf if up else -np.inf))


def volumes():
    """(vol_id, kind, vol [nz, ny, nx])."""
    rng = np.random.default_rng(20)
    out = []

    def shape(d):
        return (d[2], d[1], d[0])

    out.append(("u8 1x1x1 constant", "u8", np.full(shape(DIMS[0]), 200, np.uint8)))
    out.append(("u8 5x3x2 uniform", "u8", rng.integers(0, 256, shape(DIMS[1])).astype(np.uint8)))
    out.append(("u8 17x9x6 two-valued", "u8", rng.choice(np.array([0, 255], np.uint8), shape(DIMS[2]), p=(0.9, 0.1))))
    out.append(("u8 24^3 constant", "u8", np.full(shape(DIMS[3]), 77, np.uint8)))
    out.append(("u8 24^3 uniform", "u8", rng.integers(0, 256, shape(DIMS[3])).astype(np.uint8)))
    out.append(("u8 33x20x7 uniform", "u8", rng.integers(0, 256, shape(DIMS[4])).astype(np.uint8)))
    out.append(("u16 5x3x2 uniform", "u16", rng.integers(0, 65536, shape(DIMS[1])).astype(np.uint16)))
    out.append(("u16 17x9x6 uniform", "u16", rng.integers(0, 65536, shape(DIMS[2])).astype(np.uint16)))
    out.append(("u16 24^3 narrow band", "u16", rng.integers(1000, 1400, shape(DIMS[3])).astype(np.uint16)))
    band = rng.integers(1000, 1400, shape(DIMS[4])).astype(np.uint16)
    band.ravel()[::37] = 0
    band.ravel()[5::41] = 65535
    out.append(("u16 33x20x7 narrow band, 0 and 65535", "u16", band))
    v = rng.uniform(-2.0, 2.0, shape(DIMS[2])).astype(np.float16)
    flat = v.ravel()
    special = [np.float16(np.nan), np.float16(np.inf), np.float16(-np.inf), np.float16(-0.0), np.float16(0.0), np.float16(6e-8), np.float16(-6e-8),
               np.float16(3e-5), np.float16(0.25), np.float16(0.75), f16_next(0.25, False), f16_next(0.75, True), f16_next(0.25, True), f16_next(0.75, False),
               np.float16(1.0), f16_next(1.0, True), f16_next(0.0, False), np.float16(-4.0), np.float16(4.0), np.float16(10.0), np.float16(20.0), np.float16(65504.0)]
    for rep in range(6):
        for k, s in enumerate(special):
            flat[(rep * 151 + k * 7 + 3) % flat.size] = s
    out.append(("f16 17x9x6 NaN, inf, -0, subnormals, domain edges", "f16", v))
    w = rng.normal(0.5, 0.4, shape(DIMS[4])).astype(np.float16)
    wf = w.ravel()
    for rep in range(9):
        for k, s in enumerate(special):
            wf[(rep * 509 + k * 13 + 1) % wf.size] = s
    wf[-1] = np.float16(-0.0)   # the last voxel of an odd dimension
    wf[-2] = np.float16(np.nan)
    out.append(("f16 33x20x7 normal with the specials", "f16", w))
    out.append(("f16 24^3 uniform", "f16", rng.uniform(-2.0, 2.0, shape(DIMS[3])).astype(np.float16)))
    out.append(("f16 5x3x2 all NaN", "f16", np.full(shape(DIMS[1]), np.nan, np.float16)))
    out.append(("f16 1x1x1 -0", "f16", np.full(shape(DIMS[0]), -0.0, np.float16)))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        out, k = [], 0
        for vol_id, kind, vol in volumes():
            nz, ny, nx = vol.shape
            for bname, box in boxes(nx, ny, nz):
                bins = BINS[k % len(BINS)]
                domain = DOMAINS[kind][(k // 2) % 4]
                out.append(Case(f"{vol_id}, {bname}, {bins} bins over {domain}", vol_id, kind, vol, box, bins, domain))
                k += 1
            # the whole volume under every domain, and under the identity's request
            for j, domain in enumerate(DOMAINS[kind]):
                bins = BINS[(k + j) % len(BINS)]
                out.append(Case(f"{vol_id}, whole, {bins} bins over {domain} (domains)", vol_id, kind, vol, None, bins, domain))
            out.append(Case(f"{vol_id}, whole, 256 bins over (0.0, 1.0) (identity)", vol_id, kind, vol, None, 256, (0.0, 1.0)))
            k += 1
        _CASES = out
    return _CASES


def box_of(c):
    nz, ny, nx = c.vol.shape
    return ((0, 0, 0), (nx, ny, nz)) if c.box is None else c.box
