"""The shared cases of vk_measure_components: volumes as small as can still break a run, a chunk of 4096 voxels, the
workgroup's table of 128 slots or a limb of the sums.  Dimensions are (nx, ny, nz); arrays are [nz, ny, nx].  A case's regions come from a
value range (source "range": the library labels it; the tests also feed the label restatement's array back in as labels_in) or from a
host array (source "labels").  The volume builders are label_cases' and split_cases'."""
import collections
import math

import numpy as np

import label_cases as LC
import split_cases as SC

INF = math.inf
MAX_VOXELS = 64 * 64 * 33
SLOTS = 128

# box: None or (x0, y0, z0, x1, y1, z1); clip: None or (lo3, hi3) -- the box is then the clip box's voxel box and the call passes VK_MEASURE_CLIP_BOX
# labels: None (source "range") or uint32 [nz, ny, nx] with max_label
Case = collections.namedtuple("Case", "name vol_id vol kind lo hi conn box clip labels max_label")


def _range(kind, vol_id, vol, name, lo, hi, conn=6, box=None, clip=None):
    d = tuple(reversed(vol.shape))
    if clip is not None:
        box = LC.clip_voxel_box(clip[0], clip[1], d)
    return Case(f"{vol_id}, [{lo}, {hi}] conn {conn}, {name}", vol_id, vol, kind, float(lo), float(hi), conn, box, clip, None, 0)


def _labelled(kind, vol_id, vol, name, labels, max_label):
    return Case(f"{vol_id}, host labels up to {max_label}, {name}", vol_id, vol, kind, 0.0, 0.0, 0, None, None, np.ascontiguousarray(labels, np.uint32), int(max_label))


def bright_noise(d, kind, seed):
    """Every voxel at or above half of the format's top: one region under any connectivity, with an intensity that varies."""
    rng = np.random.default_rng(seed)
    if kind == "f16":
        return rng.uniform(0.5, 2.0, LC.shape(d)).astype(np.float16)
    top = LC.TOP[kind]
    return rng.integers(top // 2 + 1, top + 1, LC.shape(d)).astype(LC.DTYPE[kind])


def f16_extremes(d, seed):
    """Halves at the ends of the format: +-65504, the smallest subnormal of both signs, -0, +-inf, NaN, among ordinary values."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-4.0, 4.0, LC.shape(d)).astype(np.float16)
    bits = v.view(np.uint16)
    pick = rng.integers(0, 14, LC.shape(d))
    for k, b in enumerate((0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x8000, 0x7C00, 0xFC00, 0x7E00, 0x03FF)):  # 65504, -65504, 2^-24, -2^-24, -0, +inf, -inf, NaN, the largest subnormal
        bits[pick == k] = b
    return v


def slabs(d, gaps=True):
    """Host labels: slabs across x that share faces -- 1 | 2 | 3 --, with a background hole, and stripes along y further up."""
    lab = np.zeros(LC.shape(d), np.uint32)
    nx = d[0]
    lab[:, :, :nx // 3] = 1
    lab[:, :, nx // 3:2 * nx // 3] = 2
    lab[:, :, 2 * nx // 3:] = 3
    if gaps:
        lab[1:3, 2:5, 1:nx - 1] = 0
        lab[d[2] // 2:, ::2, :] = 4  # rows of 4 between rows of 1 | 2 | 3: faces across y, runs of a whole row
    return lab


_CACHE = []


def cases():
    if _CACHE:
        return _CACHE
    out = []
    # odd dimensions that end inside a tile and inside a chunk; nx < 64 and no divisor of 64: a wave spans several rows
    for kind in ("u8", "u16", "f16"):
        d = (37, 21, 19)
        vol, vid = LC.noise(d, kind, 3 + len(kind)), f"{kind} {d} uniform noise"
        for conn in (6, 26):
            out.append(_range(kind, vid, vol, "odd dimensions", 0.5, INF, conn))
        out.append(_range(kind, vid, vol, "a box", 0.4, INF, 18, box=(3, 2, 1, 30, 18, 15)))
        out.append(_range(kind, vid, vol, "the clip box", 0.4, INF, 6, clip=((0.1, 0.0, 0.2), (0.9, 0.7, 1.0))))
        out.append(_range(kind, vid, vol, "an empty box", 0.5, INF, 6, box=(3, 2, 1, 3, 9, 5)))
        d = (35, 19, 17)
        out.append(_range(kind, f"{kind} {d} percolation at density 0.31", LC.percolation(d, kind, 6), "regions of every size", 0.5, INF, {"u8": 6, "u16": 18, "f16": 26}[kind]))
    for d in ((5, 7, 40), (3, 50, 11), (70, 9, 7), (1, 1, 70), (130, 3, 5)):
        out.append(_range("u8", f"u8 {d} uniform noise", LC.noise(d, "u8", sum(d)), "short rows", 0.35, INF, 6))
    # one region that fills the largest volume: many chunks, one hot record, runs of 64 and runs cut by row ends
    for kind in ("u8", "f16"):
        d = (64, 64, 33)
        out.append(_range(kind, f"{kind} {d} every voxel bright", bright_noise(d, kind, 8), "one region fills the volume", 0.45, INF, 6))
    d = (61, 33, 31)
    out.append(_range("u16", f"u16 {d} every voxel bright", bright_noise(d, "u16", 9), "one region fills the volume", 0.45, INF, 26))
    # a region on every border of the volume, and of a box
    vol, vid = np.full(LC.shape((37, 21, 11)), 255, np.uint8), "u8 (37, 21, 11) constant, all foreground"
    out.append(_range("u8", vid, vol, "a region on every border", 0.5, INF, 6))
    out.append(_range("u8", vid, vol, "a region on every border of a box", 0.5, INF, 6, box=(3, 2, 1, 30, 18, 9)))
    # isolated voxels on a 3-D checkerboard: 6912 regions under 6, far more than slots; one region under 26
    for kind in ("u8", "u16"):
        d = (24, 24, 24)
        vol, vid = LC.checkerboard(d, kind), f"{kind} {d} checkerboard"
        out.append(_range(kind, vid, vol, "isolated voxels", 0.5, INF, 6))
        out.append(_range(kind, vid, vol, "one region through the corners", 0.5, INF, 26))
    # R16_UNORM: a region entirely 65535 -- the squares
    d = (37, 23, 21)
    out.append(_range("u16", f"u16 {d} two balls, a wire and a speck", LC._two_valued(SC.fixed_mask(), "u16"), "every voxel 65535", 0.5, INF, 6))
    out.append(_range("u8", f"u8 {d} two balls, a wire and a speck", LC._two_valued(SC.fixed_mask(), "u8"), "section 27's fixed case", 0.5, INF, 6))
    # R16F: the ends of the format
    d = (37, 21, 11)
    vol, vid = f16_extremes(d, 5), f"f16 {d} +-65504, subnormals, -0, inf, NaN"
    for lo, hi, conn in ((-INF, INF, 6), (0.0, INF, 26), (-INF, -0.0, 6), (60000.0, INF, 26), (-1.0, 1.0, 6)):
        out.append(_range("f16", vid, vol, "extremes", lo, hi, conn))
    big = np.full(LC.shape((64, 33, 17)), 65504.0, np.float16)
    big[::2] = np.float16(-65504.0)
    out.append(_range("f16", "f16 (64, 33, 17) planes of +-65504", big, "the widest sums", -INF, INF, 6))
    # host labels: regions that share faces, unused ids, NaN and inf under a label, a region with no finite voxel
    for kind in ("u8", "u16", "f16"):
        d = (37, 21, 11)
        vol = f16_extremes(d, 5) if kind == "f16" else LC.noise(d, kind, 21)
        out.append(_labelled(kind, f"{kind} {d} under slabs", vol, "regions that share faces", slabs(d), 4))
        out.append(_labelled(kind, f"{kind} {d} under slabs", vol, "unused ids", slabs(d) * 3, 14))
    d = (37, 21, 11)
    vol = f16_extremes(d, 5)
    bits = vol.view(np.uint16)
    lab = np.zeros(vol.shape, np.uint32)
    lab[(bits & 0x7C00) == 0x7C00] = 2                       # every NaN and inf, and nothing else
    lab[(bits == 0x8000) | (bits == 0x0001)] = 1
    out.append(_labelled("f16", f"f16 {d} +-65504, subnormals, -0, inf, NaN", vol, "a region with no finite voxel", lab, 3))
    rng = np.random.default_rng(12)
    d = (45, 13, 9)
    out.append(_labelled("u8", f"u8 {d} uniform noise", LC.noise(d, "u8", 4), "a caller's scattered segmentation", rng.integers(0, 300, LC.shape(d)) * (rng.random(LC.shape(d)) < 0.7), 320))
    one = np.ones(LC.shape((64, 64, 5)), np.uint32)
    out.append(_labelled("u16", "u16 (64, 64, 5) every voxel bright", bright_noise((64, 64, 5), "u16", 2), "one label everywhere", one, 1))
    assert len({c.name for c in out}) == len(out)
    for c in out:
        c.vol.setflags(write=False)
        if c.labels is not None:
            c.labels.setflags(write=False)
    _CACHE.extend(out)
    return _CACHE
