"""The request and the result of the local-thickness pass (vk_local_thickness): Context.local_thickness is built on these."""
import math

from . import _native as N


def thickness_request(lo, hi=float("inf"), max_radius: float = 16.0, spacing=(1, 1, 1), box=None, gain=None, fill_out: float = 0.0, install: bool = False) -> N.VkThicknessRequest:
    """A VkThicknessRequest.  max_radius: the cap of the radius in the units of spacing, finite, >= 1.  spacing: three integers
    1 .. DIST_MAX_SPACING (x, y, z).  gain: None asks for the automatic gain (the thickest place stores full scale), else finite and
    > 0.  Raises ValueError for what cannot be put into the struct; the library refuses the rest."""
    spacing = tuple(spacing)
    if len(spacing) != 3 or any(int(s) != s or not 1 <= int(s) <= N.DIST_MAX_SPACING for s in spacing):
        raise ValueError("spacing: three integers 1 .. DIST_MAX_SPACING (x, y, z)")
    max_radius = float(max_radius)
    if not (math.isfinite(max_radius) and max_radius >= 1.0):
        raise ValueError("max_radius: finite, >= 1")
    if gain is not None and not (math.isfinite(float(gain)) and float(gain) > 0.0):
        raise ValueError("gain: None (automatic), or finite and > 0")
    req = N.VkThicknessRequest()
    req.lo, req.hi, req.max_radius, req.fill_out = float(lo), float(hi), max_radius, float(fill_out)
    req.gain = 0.0 if gain is None else float(gain)
    req.flags = (N.THICK_CLIP_BOX if box == "clip" else 0) | (N.THICK_INSTALL if install else 0)
    req.spacing[0], req.spacing[1], req.spacing[2] = (int(s) for s in spacing)
    return req


class Thickness:
    """The totals of Context.local_thickness: n_foreground, max_t2, n_saturated, sum_t2 and the gain used, the derived max_thickness
    (2 sqrt(max_t2), in the units of spacing) and mean_t2 (sum_t2 / n_foreground; 0 for an empty set), and, where asked for, t2 (uint32
    [nz, ny, nx]: the squared radius per voxel) and dense (the stored map [nz, ny, nx])."""

    def __init__(self, res: N.VkThicknessResult, t2=None, dense=None):
        self.n_foreground, self.max_t2, self.n_saturated, self.sum_t2 = int(res.n_foreground), int(res.max_t2), int(res.n_saturated), int(res.sum_t2)
        self.gain = float(res.gain)
        self.max_thickness = 2.0 * math.sqrt(self.max_t2)
        self.mean_t2 = self.sum_t2 / self.n_foreground if self.n_foreground else 0.0
        self.t2, self.dense = t2, dense

    def __repr__(self):
        return "Thickness(n_foreground=%d, max_thickness=%.6g, n_saturated=%d, gain=%.6g)" % (self.n_foreground, self.max_thickness, self.n_saturated, self.gain)
