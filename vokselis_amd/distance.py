"""The request of the distance pass (vk_distance_transform): Context.distance_transform and Context.morph_volume are built on it."""
import math

from . import _native as N

DISTANCE_OPS = {"outside": N.DIST_OUTSIDE, "inside": N.DIST_INSIDE}
MORPH_OPS = {"dilate": N.DIST_DILATE, "erode": N.DIST_ERODE, "close": N.DIST_CLOSE, "open": N.DIST_OPEN}
OPS = dict(DISTANCE_OPS, **MORPH_OPS)


def default_fill_in(lo, hi) -> float:
    """The sample value a voxel takes when it joins [lo, hi] and the caller names none: hi where it is finite, else max(lo, 1) -- a value
    of the range whatever the format rounds it to."""
    lo, hi = float(lo), float(hi)
    if math.isfinite(hi):
        return hi
    return max(lo, 1.0) if math.isfinite(lo) else 1.0


def distance_request(lo, hi=float("inf"), op: str = "outside", radius: float = 0.0, spacing=(1, 1, 1), fill_in=None, fill_out: float = 0.0, install: bool = False,
                     box=None) -> N.VkDistanceRequest:
    """A VkDistanceRequest.  op: "outside", "inside" (radius must stay 0), "dilate", "erode", "close" or "open".  spacing: three integers
    1 .. DIST_MAX_SPACING (x, y, z).  Raises ValueError for what cannot be put into the struct; the library refuses the rest."""
    if op not in OPS:
        raise ValueError('op: "outside", "inside", "dilate", "erode", "close" or "open"')
    spacing = tuple(spacing)
    if len(spacing) != 3 or any(int(s) != s or not 1 <= int(s) <= N.DIST_MAX_SPACING for s in spacing):
        raise ValueError("spacing: three integers 1 .. DIST_MAX_SPACING (x, y, z)")
    radius = float(radius)
    if not (math.isfinite(radius) and 0.0 <= radius <= N.DIST_MAX_RADIUS):
        raise ValueError("radius: finite, 0 .. DIST_MAX_RADIUS")
    req = N.VkDistanceRequest()
    req.lo, req.hi, req.op, req.radius = float(lo), float(hi), OPS[op], radius
    req.flags = (N.DIST_CLIP_BOX if box == "clip" else 0) | (N.DIST_INSTALL if install else 0)
    req.spacing[0], req.spacing[1], req.spacing[2] = (int(s) for s in spacing)
    req.fill_in = default_fill_in(lo, hi) if fill_in is None else float(fill_in)
    req.fill_out = float(fill_out)
    return req
