"""The request and the result of the skeleton pass (vk_skeletonize): Context.skeletonize is built on these."""
import math

from . import _native as N

MODES = {"curve": N.SKEL_CURVE, "kernel": N.SKEL_KERNEL}


def skeleton_request(lo, hi=float("inf"), mode="curve", max_iterations: int = 0, fill_in=None, fill_out: float = 0.0, box=None, install: bool = True) -> N.VkSkeletonRequest:
    """A VkSkeletonRequest.  mode: "curve" (line ends stay: centre lines) or "kernel" (no end condition: the ultimate homotopic kernel);
    max_iterations: 0 thins until an iteration deletes nothing; fill_in: None keeps the stored value on the skeleton, a number stores
    that sample value there (SKEL_FILL_IN); fill_out: the sample value everywhere else.  Raises ValueError for what cannot be put into
    the struct; the library refuses the rest."""
    if mode not in MODES:
        raise ValueError("mode: 'curve' or 'kernel'")
    if int(max_iterations) != max_iterations or not 0 <= int(max_iterations) < 2 ** 32:
        raise ValueError("max_iterations: an integer 0 .. 2^32 - 1 (0: until nothing is deleted)")
    req = N.VkSkeletonRequest()
    req.lo, req.hi, req.fill_out = float(lo), float(hi), float(fill_out)
    req.mode, req.max_iterations = MODES[mode], int(max_iterations)
    req.flags = (N.SKEL_CLIP_BOX if isinstance(box, str) and box == "clip" else 0) | (N.SKEL_INSTALL if install else 0) | (N.SKEL_FILL_IN if fill_in is not None else 0)
    req.fill_in = float(fill_in) if fill_in is not None else 0.0
    return req


def link_offsets():
    """The 13 offsets (dx, dy, dz) of Skeleton.links: those above the centre in the order of the 3 x 3 x 3 neighbourhood."""
    return [(o % 3 - 1, o // 3 % 3 - 1, o // 9 - 1) for o in range(14, 27)]


class Skeleton:
    """The totals of Context.skeletonize -- n_foreground (the range's voxels), n_skeleton (what is left of them), the voxels of the
    skeleton by class: n_isolated (no neighbour on the skeleton), n_end (one), n_regular (two), n_junction (three or more), links (per
    offset of link_offsets() the 26-adjacent pairs of skeleton voxels), iterations (those that deleted something) and converged -- and
    length(spacing); where asked for, classes (uint8 [nz, ny, nx]: 0 off the skeleton, SKEL_ISOLATED, SKEL_END, SKEL_REGULAR,
    SKEL_JUNCTION) and dense (the stored volume [nz, ny, nx])."""

    def __init__(self, res: N.VkSkeletonResult, classes=None, dense=None):
        for name in ("n_foreground", "n_skeleton", "n_isolated", "n_end", "n_regular", "n_junction", "iterations"):
            setattr(self, name, int(getattr(res, name)))
        self.links = tuple(int(v) for v in res.links)
        self.converged = bool(res.converged)
        self.classes, self.dense = classes, dense

    def length(self, spacing=(1.0, 1.0, 1.0)) -> float:
        """sum_j links[j] sqrt(sum_c (spacing[c] d_c)^2): the centre-line length in the units of the spacing.  Every adjacent pair counts,
        so the sum over-counts inside junction clumps, where a voxel is adjacent to more than two others."""
        sx, sy, sz = (float(s) for s in spacing)
        return sum(n * math.sqrt((sx * dx) ** 2 + (sy * dy) ** 2 + (sz * dz) ** 2) for n, (dx, dy, dz) in zip(self.links, link_offsets()))

    def __repr__(self):
        return "Skeleton(n_foreground=%d, n_skeleton=%d, n_end=%d, n_junction=%d, n_isolated=%d, iterations=%d, converged=%s)" % (
            self.n_foreground, self.n_skeleton, self.n_end, self.n_junction, self.n_isolated, self.iterations, self.converged)
