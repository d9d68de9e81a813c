"""The shared cases of vk_volume_resample, from a fixed seed: source extents from {1, 2, 3, 5, 37, 70}, output
extents from {1, 2, 3, 7, 64, 67, 130} -- 64 is exactly the edge of the workgroup's tile (64 x 4), 37, 67, 70 and 130 are no multiple
of the wave or of either edge -- ratios up, down, mixed per axis and exactly 16; the whole volume, a one-voxel box, a box touching each face, the clip box; the
three modes; every format pair with and without a window (narrower than one LSB of the source, clamping both ends); noise, a ramp, the
constants 0 and the maximum, a label-like volume of few values, f16 data with NaN, both infinities, subnormals and 65504.
Dimensions are (nx, ny, nz); arrays are [nz, ny, nx]."""
import collections

import numpy as np

SRC = (1, 2, 3, 5, 37, 70)
OUT = (1, 2, 3, 7, 64, 67, 130)
MODES = ("nearest", "linear", "area")
KINDS = ("u8", "u16", "f16")
DTYPE = {"u8": np.uint8, "u16": np.uint16, "f16": np.float16}
FMT = {"u8": 0, "f16": 1, "u16": 3}
TOP = {"u8": 255, "u16": 65535, "f16": 1.0}
MAX_RATIO = 16
MAX_VOXELS = 70 ** 3
MAX_OUT_VOXELS = 1 << 20  # keeps the per-voxel restatement and the whole-array reference to seconds over the list

# box: (x0, y0, z0, x1, y1, z1), always explicit; clip: None or (lo3, hi3) -- the call then passes VK_RESAMPLE_CLIP_BOX and no box, and
# `box` is the clip box's voxel box.  dims: the output extents, all > 0.  out: the output kind.  window: None or (lo, hi).
# refused: None, or the status (-1, -5) the library answers with.
Case = collections.namedtuple("Case", "name vol_id vol kind box clip mode dims out window refused")


def shape(d):
    return (d[2], d[1], d[0])


def clip_voxel_box(lo, hi, dims):
    """The voxels whose centre (i + 0.5) / n, in double, lies in [lo, hi] as f32: vk_volume_histogram's rule for the clip box."""
    out = []
    for a in range(3):
        l, h, n = float(np.float32(lo[a])), float(np.float32(hi[a])), dims[a]
        inside = [i for i in range(n) if l <= (i + 0.5) / n <= h]
        out.append((inside[0], inside[-1] + 1) if inside else (0, 0))
    return (out[0][0], out[1][0], out[2][0], out[0][1], out[1][1], out[2][1])


def noise(d, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "f16":
        return rng.uniform(-1.0, 2.0, shape(d)).astype(np.float16)
    return rng.integers(0, TOP[kind] + 1, shape(d)).astype(DTYPE[kind])


def ramp(d, kind):
    z, y, x = np.indices(shape(d))
    t = (x + 2 * y + 3 * z).astype(np.float64)
    t = t / max(1.0, float(t.max()))
    return (t * TOP[kind]).astype(DTYPE[kind]) if kind == "f16" else np.rint(t * TOP[kind]).astype(DTYPE[kind])


def constant(d, kind, value):
    return np.full(shape(d), value, DTYPE[kind])


def labels(d, kind, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([0, 1, 2, 7, TOP[kind]] if kind != "f16" else [0.0, 1.0, 2.0, 7.0, 0.5]).astype(DTYPE[kind])
    coarse = rng.integers(0, len(vals), tuple((n + 3) // 4 for n in shape(d)))
    return vals[np.kron(coarse, np.ones((4, 4, 4), np.int64))[:d[2], :d[1], :d[0]]]


def f16_edges(d, seed):
    """Halves of every class: NaN with payloads, both infinities, subnormals, zeros of both signs, 65504, ordinary values."""
    rng = np.random.default_rng(seed)
    special = np.array([0x7e00, 0x7c01, 0xfe12, 0x7c00, 0xfc00, 0x0001, 0x8001, 0x03ff, 0x0000, 0x8000, 0x7bff, 0xfbff, 0x3c00, 0x0400], np.uint16)
    v = rng.uniform(-4.0, 4.0, shape(d)).astype(np.float16).view(np.uint16)
    pick = rng.random(shape(d)) < 0.25
    v = np.where(pick, special[rng.integers(0, len(special), shape(d))], v).astype(np.uint16)
    return v.view(np.float16)


_VOLUMES = None


def volumes():
    """(vol_id, kind, array): every source extent on every axis, one voxel to 70^3."""
    global _VOLUMES
    if _VOLUMES is None:
        _VOLUMES = _volumes()
    return _VOLUMES


def _volumes():
    out = []
    for kind in KINDS:
        out.append((f"{kind} noise (70, 37, 5)", kind, noise((70, 37, 5), kind, 11)))
        out.append((f"{kind} ramp (37, 70, 3)", kind, ramp((37, 70, 3), kind)))
        out.append((f"{kind} labels (37, 37, 37)", kind, labels((37, 37, 37), kind, 12)))
        out.append((f"{kind} zero (5, 3, 2)", kind, constant((5, 3, 2), kind, 0)))
        out.append((f"{kind} maximum (3, 5, 37)", kind, constant((3, 5, 37), kind, TOP[kind] if kind != "f16" else 65504.0)))
        out.append((f"{kind} noise (1, 1, 1)", kind, noise((1, 1, 1), kind, 13)))
        out.append((f"{kind} noise (2, 70, 1)", kind, noise((2, 70, 1), kind, 14)))
        out.append((f"{kind} noise (3, 2, 5)", kind, noise((3, 2, 5), kind, 19)))
    out.append(("u8 noise (70, 70, 70)", "u8", noise((70, 70, 70), "u8", 15)))
    out.append(("u16 noise (37, 70, 70)", "u16", noise((37, 70, 70), "u16", 16)))
    out.append(("f16 edges (37, 5, 3)", "f16", f16_edges((37, 5, 3), 17)))
    out.append(("f16 edges (70, 37, 37)", "f16", f16_edges((70, 37, 37), 18)))
    return out


def _dims_of(vol):
    return (vol.shape[2], vol.shape[1], vol.shape[0])


def _boxes(d, rng):
    """(label, box, clip) choices of a volume of dims d."""
    out = [("whole", (0, 0, 0) + tuple(d), None)]
    p = tuple(int(rng.integers(0, n)) for n in d)
    out.append(("one voxel", p + tuple(v + 1 for v in p), None))
    for a in range(3):
        for side in (0, 1):
            lo, hi = [n // 4 if n > 3 else 0 for n in d], [n - n // 4 if n > 3 else n for n in d]
            if side == 0:
                lo[a] = 0
            else:
                hi[a] = d[a]
            out.append((f"touches {'xyz'[a]}{'-+'[side]}", tuple(lo) + tuple(hi), None))
    lo3, hi3 = (0.13, 0.0, 0.21), (0.81, 0.77, 1.0)
    cb = clip_voxel_box(lo3, hi3, d)
    if min(cb[3] - cb[0], cb[4] - cb[1], cb[5] - cb[2]) > 0:
        out.append(("clip", cb, (lo3, hi3)))
    return out


def _windows(kind):
    """Window choices for a source kind: None, an ordinary one, one narrower than one LSB of the source, one clamping both ends."""
    lsb = {"u8": 1.0 / 255.0, "u16": 1.0 / 65535.0, "f16": 2.0 ** -11}[kind]
    return [None, (0.1, 0.6), (0.5, 0.5 + 0.3 * lsb), (0.4, 0.45), (-0.25, 1.5)]


def _fits(mode, nb, n):
    return mode != "area" or all(b <= MAX_RATIO * m for b, m in zip(nb, n))


def _name(vol_id, label, box, mode, dims, out, window):
    w = "" if window is None else f", window {window[0]:g} .. {window[1]:g}"
    return f"{vol_id}, {label} box {box}, {mode} to {dims} {out}{w}"


def _build():
    rng = np.random.default_rng(20261020)
    out = []
    for vol_id, kind, vol in volumes():
        d = _dims_of(vol)
        boxes = _boxes(d, rng)
        per_volume = 10 if vol.size > 50 else 5
        k = 0
        while k < per_volume:
            label, box, clip = boxes[int(rng.integers(0, len(boxes)))] if k >= 3 else boxes[(0, 2, len(boxes) - 1)[k]]
            nb = (box[3] - box[0], box[4] - box[1], box[5] - box[2])
            mode = MODES[k % 3] if k < 3 else MODES[int(rng.integers(0, 3))]
            dims = tuple(int(OUT[int(rng.integers(0, len(OUT)))]) for _ in range(3))
            if int(rng.integers(0, 6)) == 0:
                dims = nb  # the box's own extents: a crop
            if not _fits(mode, nb, dims) or dims[0] * dims[1] * dims[2] > MAX_OUT_VOXELS:
                continue
            okind = kind if int(rng.integers(0, 2)) == 0 else KINDS[int(rng.integers(0, 3))]
            ws = _windows(kind)
            window = ws[int(rng.integers(0, len(ws)))] if int(rng.integers(0, 2)) else None
            out.append(Case(_name(vol_id, label, box, mode, dims, okind, window), vol_id, vol, kind, box, clip, mode, dims, okind, window, None))
            k += 1
    by_id = {v[0]: v for v in volumes()}
    # every format pair under every mode, with and without a window, on one volume per kind
    for kind in KINDS:
        vol_id, _, vol = by_id[f"{kind} noise (70, 37, 5)"]
        d = _dims_of(vol)
        for okind in KINDS:
            for mode in MODES:
                for window in (None, (0.25, 0.75)):
                    dims = {"nearest": (67, 7, 3), "linear": (130, 64, 7), "area": (7, 3, 2)}[mode]
                    out.append(Case(_name(vol_id, "whole", (0, 0, 0) + d, mode, dims, okind, window), vol_id, vol, kind, (0, 0, 0) + d, None, mode, dims, okind, window, None))
    # the identity, the ratio of exactly 16, and 16 plus a voxel
    for kind in KINDS:
        for vid in (f"{kind} noise (70, 37, 5)", f"{kind} labels (37, 37, 37)") + (("f16 edges (70, 37, 37)",) if kind == "f16" else ()):
            vol_id, _, vol = by_id[vid]
            d = _dims_of(vol)
            for mode in MODES:
                out.append(Case(_name(vol_id, "whole", (0, 0, 0) + d, mode, d, kind, None) + " (identity)", vol_id, vol, kind, (0, 0, 0) + d, None, mode, d, kind, None, None))
    for kind, vid in (("u8", "u8 noise (70, 70, 70)"), ("u16", "u16 noise (37, 70, 70)"), ("f16", "f16 edges (70, 37, 37)")):
        vol_id, _, vol = by_id[vid]
        d = _dims_of(vol)
        b16 = (3, 1, 2, 35, 33, 34)      # 32^3 -> (2, 2, 2): 16 exactly on every axis
        out.append(Case(_name(vol_id, "ratio 16", b16, "area", (2, 2, 2), kind, None), vol_id, vol, kind, b16, None, "area", (2, 2, 2), kind, None, None))
        b48 = (1, 0, 5, 1 + min(48, d[0] - 1), 16, 37)  # (48 or 36, 16, 32) -> (3, 1, 2)
        out.append(Case(_name(vol_id, "ratio 16 mixed", b48, "area", (3, 1, 2), kind, None), vol_id, vol, kind, b48, None, "area", (3, 1, 2), kind, None, None))
        b17 = (3, 1, 2, 35, 34, 34)      # y: 33 -> 2
        out.append(Case(_name(vol_id, "ratio 16 plus a voxel", b17, "area", (2, 2, 2), kind, None), vol_id, vol, kind, b17, None, "area", (2, 2, 2), kind, None, -5))
        out.append(Case(_name(vol_id, "ratio 16 plus a voxel", b17, "linear", (2, 2, 2), kind, None), vol_id, vol, kind, b17, None, "linear", (2, 2, 2), kind, None, None))
    # AREA by 2, 3 and 4 on every axis: on integer data the exact block means; the ratios the unrolled kernels take
    for kind in KINDS:
        vol_id, _, vol = by_id[f"{kind} noise (70, 37, 5)"]
        for f in (2, 3, 4):
            box = (2, 1, 0, 2 + 12 * 5, 1 + 12 * 3, 4) if f != 3 else (2, 1, 0, 62, 37, 3)
            nb = (box[3] - box[0], box[4] - box[1], box[5] - box[2])
            fz = {2: 2, 3: 3, 4: 4}[f]
            dims = (nb[0] // f, nb[1] // f, nb[2] // fz)
            out.append(Case(_name(vol_id, f"blocks of {f}", box, "area", dims, kind, None), vol_id, vol, kind, box, None, "area", dims, kind, None, None))
    names = [c.name for c in out]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1][:3]
    for c in out:
        c.vol.setflags(write=False)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def runnable():
    return [c for c in cases() if c.refused is None]
