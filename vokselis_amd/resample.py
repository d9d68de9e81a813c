"""The request of the resample pass (vk_volume_resample): Context.resample_volume, crop_volume, downsample_volume and isotropic_volume
are built on these.  resample_request validates without a device and mirrors the library's refusals of a request; what depends on the
volume (the box, the AREA ratio, the layout of an install) the library refuses."""
import math

import numpy as np

from . import _native as N
from .label import voxel_box

MODES = {"nearest": N.RESAMPLE_NEAREST, "linear": N.RESAMPLE_LINEAR, "area": N.RESAMPLE_AREA}
FORMATS = {None: N.RESAMPLE_KEEP_FORMAT, "u8": N.FMT_R8_UNORM, "u16": N.FMT_R16_UNORM, "f16": N.FMT_R16_FLOAT}
SCALE = {N.FMT_R8_UNORM: 255.0, N.FMT_R16_UNORM: 65535.0, N.FMT_R16_FLOAT: 1.0}
DTYPE = {N.FMT_R8_UNORM: np.uint8, N.FMT_R16_UNORM: np.uint16, N.FMT_R16_FLOAT: np.float16}
MAX_EXTENT = 65535


def _format(fmt) -> int:
    if fmt in FORMATS:
        return FORMATS[fmt]
    if fmt == N.FMT_RGBA16F_PAIR and not isinstance(fmt, bool):
        raise ValueError("resample: RGBA16F_PAIR is no output format")
    if isinstance(fmt, int) and not isinstance(fmt, bool) and fmt in (N.RESAMPLE_KEEP_FORMAT, N.FMT_R8_UNORM, N.FMT_R16_UNORM, N.FMT_R16_FLOAT):
        return fmt
    raise ValueError('resample: fmt is None (keep), "u8", "u16", "f16" or FMT_R8_UNORM / FMT_R16_UNORM / FMT_R16_FLOAT')


def value_map(fmt_in: int, fmt_out: int, lo: float = 0.0, hi: float = 1.0):
    """The value map's (a, b) as f32: a = S_out / ((hi - lo) S_in), b = -lo S_out / (hi - lo), in double, each rounded once."""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    with np.errstate(over="ignore"):
        return np.float32(SCALE[fmt_out] / ((hi - lo) * SCALE[fmt_in])), np.float32(-lo * SCALE[fmt_out] / (hi - lo))


def resample_request(dims=None, mode: str = "linear", fmt=None, window=None, layout=None, box=None, install: bool = True, out: bool = False) -> N.VkResampleRequest:
    """A VkResampleRequest.  dims: None (the box's extents) or (nx, ny, nz), 0 or None per axis keeps that axis; mode: "nearest", "linear"
    or "area"; fmt: None (the volume's), "u8", "u16", "f16" or a FMT_ constant; window: None or (lo, hi) in sample values; layout: None
    (LAYOUT_AUTO) or a LAYOUT_ constant; box: None, "clip" or ((x0, y0, z0), (x1, y1, z1)).  Raises ValueError with the library's
    reasons: an unknown mode or format, an extent above 65535, a window that is not finite or has lo >= hi, neither install nor out."""
    if mode not in MODES:
        raise ValueError('resample: mode is "nearest", "linear" or "area"')
    req = N.VkResampleRequest()
    req.mode = MODES[mode]
    req.format = _format(fmt)
    d = (0, 0, 0) if dims is None else tuple(0 if v is None else int(v) for v in dims)
    if len(d) != 3 or min(d) < 0:
        raise ValueError("resample: dims is None or three extents >= 0 (0: the axis keeps the box's extent)")
    if max(d) > MAX_EXTENT:
        raise ValueError("resample: an output extent is above 65535")
    req.dims[0], req.dims[1], req.dims[2] = d
    voxel_box(box)  # (its own refusals)
    flags = (N.RESAMPLE_INSTALL if install else 0) | (N.RESAMPLE_CLIP_BOX if box == "clip" else 0)
    if window is not None:
        lo, hi = (float(v) for v in window)
        with np.errstate(over="ignore"):
            lo32, hi32 = float(np.float32(lo)), float(np.float32(hi))
        if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(lo32) and math.isfinite(hi32)):
            raise ValueError("resample: the window's lo or hi is not finite")
        req.lo, req.hi = lo, hi
        if not req.lo < req.hi:  # (as the library compares them: rounded to f32)
            raise ValueError("resample: the window needs lo < hi")
        flags |= N.RESAMPLE_WINDOW
    if not (install or out):
        raise ValueError("resample: neither out nor install: the result would go nowhere")
    lay = N.LAYOUT_AUTO if layout is None else int(layout)
    if not N.LAYOUT_AUTO <= lay <= N.LAYOUT_STAGED:
        raise ValueError("resample: unknown layout")
    req.layout = lay
    req.flags = flags
    return req


def downsample_dims(box_dims, factor) -> tuple:
    """ceil(n / factor) per axis; factor: one integer >= 1 or three."""
    f = tuple(factor) if isinstance(factor, (tuple, list, np.ndarray)) else (factor, factor, factor)
    if len(f) != 3 or any(int(v) != v or int(v) < 1 for v in f):
        raise ValueError("downsample: factor is an integer >= 1, or three of them")
    return tuple(-(-int(n) // int(v)) for n, v in zip(box_dims, f))


def isotropic_dims(box_dims, spacing) -> tuple:
    """max(1, round(n_c * spacing_c / min(spacing))) per axis: the extents at which every voxel has the finest spacing of the three."""
    s = tuple(float(v) for v in spacing)
    if len(s) != 3 or not all(math.isfinite(v) and v > 0.0 for v in s):
        raise ValueError("isotropic: spacing is three finite numbers > 0")
    return tuple(max(1, int(round(int(n) * v / min(s)))) for n, v in zip(box_dims, s))
