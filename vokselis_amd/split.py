"""The request and the result of the split pass (vk_split_components): Context.split_components is built on these."""
import math

from . import _native as N
from .label import Components


def split_request(lo, hi=float("inf"), radius: float = 0.0, spacing=(1, 1, 1), connectivity: int = 6, box=None, fill_out: float = 0.0, install: bool = False) -> N.VkSplitRequest:
    """A VkSplitRequest.  radius: the erosion radius in the units of spacing, finite, 0 .. DIST_MAX_RADIUS.  spacing: three integers
    1 .. DIST_MAX_SPACING (x, y, z).  Raises ValueError for what cannot be put into the struct; the library refuses the rest."""
    spacing = tuple(spacing)
    if len(spacing) != 3 or any(int(s) != s or not 1 <= int(s) <= N.DIST_MAX_SPACING for s in spacing):
        raise ValueError("spacing: three integers 1 .. DIST_MAX_SPACING (x, y, z)")
    radius = float(radius)
    if not (math.isfinite(radius) and 0.0 <= radius <= N.DIST_MAX_RADIUS):
        raise ValueError("radius: finite, 0 .. DIST_MAX_RADIUS")
    req = N.VkSplitRequest()
    req.lo, req.hi, req.connectivity, req.radius, req.fill_out = float(lo), float(hi), int(connectivity), radius, float(fill_out)
    req.flags = (N.SPLIT_CLIP_BOX if box == "clip" else 0) | (N.SPLIT_INSTALL if install else 0)
    req.spacing[0], req.spacing[1], req.spacing[2] = (int(s) for s in spacing)
    return req


class Regions(Components):
    """The regions of Context.split_components in id order, shaped like Components -- n, sizes, first (a region's ANCHOR: the smallest
    linear index of its marker component, or of the region itself where no marker reached it), boxes, largest(k), n_foreground, labels --
    plus n_markers, n_marker_voxels, n_residue_regions, n_residue_voxels, n_cut and rounds, and dense (the cut volume, or None)."""

    def __init__(self, table, res: N.VkSplitResult, labels=None, dense=None):
        self.n_regions = int(res.n_regions)  # all of them; n, below, is how many the table holds (fewer only after an install of more than its room)
        super().__init__(table, min(self.n_regions, len(table)), int(res.n_foreground), labels)
        self.n_markers, self.n_marker_voxels = int(res.n_markers), int(res.n_marker_voxels)
        self.n_residue_regions, self.n_residue_voxels = int(res.n_residue_regions), int(res.n_residue_voxels)
        self.n_cut, self.rounds = int(res.n_cut), int(res.rounds)
        self.dense = dense

    def __repr__(self):
        return "Regions(n=%d, n_markers=%d, n_residue_regions=%d, n_cut=%d, rounds=%d)" % (self.n, self.n_markers, self.n_residue_regions, self.n_cut, self.rounds)
