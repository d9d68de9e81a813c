"""The request and the result of the connected-components pass (vk_label_components): Context.label_components and keep_components are
built on these.  voxel_of turns a position in unit-cube coordinates -- Context.pick(x, y).pos -- into the voxel that holds it: a seed."""
import math

import numpy as np

from . import _native as N

KEEP = {"all": N.LABEL_KEEP_ALL, "largest": N.LABEL_KEEP_LARGEST, "min_size": N.LABEL_KEEP_MIN_SIZE, "seeds": N.LABEL_KEEP_SEEDS}


def voxel_of(pos, dims) -> tuple:
    """The voxel (x, y, z) of a volume of dims = (nx, ny, nz) that holds the unit-cube position `pos`: min(floor(pos_c * n_c), n_c - 1)
    per axis -- texel centres at (i + 0.5) / n, the convention of the mesh and of Hit.pos.  Raises ValueError outside [0, 1]."""
    pos, dims = tuple(float(v) for v in pos), tuple(int(v) for v in dims)
    if len(pos) != 3 or len(dims) != 3 or min(dims) < 1:
        raise ValueError("voxel_of: a position and dims of three components each, dims >= 1")
    if not all(math.isfinite(p) and 0.0 <= p <= 1.0 for p in pos):
        raise ValueError("voxel_of: the position lies outside the unit cube")
    return tuple(min(int(math.floor(p * n)), n - 1) for p, n in zip(pos, dims))


def voxel_box(box):
    """None, "clip" (None: the flag says it) or ((x0, y0, z0), (x1, y1, z1)) as a VkVoxelBox."""
    if box is None or isinstance(box, str):
        if box not in (None, "clip"):
            raise ValueError('box: None, "clip" or ((x0, y0, z0), (x1, y1, z1))')
        return None
    lo, hi = (tuple(int(v) for v in c) for c in box)
    if len(lo) != 3 or len(hi) != 3 or min(lo + hi) < 0:
        raise ValueError("box: two triples of voxel indices >= 0")
    return N.VkVoxelBox(*lo, *hi)


def label_request(lo, hi=float("inf"), connectivity: int = 6, box=None, keep: str = "all", count: int = 1, seeds=(), invert: bool = False, fill: float = 0.0,
                  install: bool = False) -> N.VkLabelRequest:
    """A VkLabelRequest.  keep: "all", "largest", "min_size" (both use count) or "seeds" (1 .. LABEL_MAX_SEEDS voxels (x, y, z)).  Raises
    ValueError for what cannot be put into the struct; the library refuses the rest."""
    if keep not in KEEP:
        raise ValueError('keep: "all", "largest", "min_size" or "seeds"')
    req = N.VkLabelRequest()
    req.lo, req.hi, req.connectivity, req.keep, req.fill = float(lo), float(hi), int(connectivity), KEEP[keep], float(fill)
    req.flags = (N.LABEL_CLIP_BOX if box == "clip" else 0) | (N.LABEL_INSTALL if install else 0) | (N.LABEL_INVERT if invert else 0)
    if keep in ("largest", "min_size"):
        if int(count) < 1:
            raise ValueError("count: >= 1")
        req.count = int(count)
    if keep == "seeds":
        seeds = [tuple(int(v) for v in s) for s in seeds]
        if len(seeds) > N.LABEL_MAX_SEEDS or any(len(s) != 3 or min(s) < 0 for s in seeds):
            raise ValueError("seeds: at most LABEL_MAX_SEEDS voxels (x, y, z) >= 0")
        req.n_seeds = len(seeds)
        for k, s in enumerate(seeds):
            req.seeds[k][0], req.seeds[k][1], req.seeds[k][2] = s
    return req


class Components:
    """The components of Context.label_components in id order (id k + 1 at index k): n, sizes (uint64), first (uint64: the smallest
    linear index x + nx (y + ny z)), boxes (uint32 [n, 6]: x0, y0, z0, x1, y1, z1, half-open), n_foreground, labels or None."""

    def __init__(self, table, n: int, n_foreground: int, labels=None):
        self.n = int(n)
        self.sizes = np.array([table[k].n_voxels for k in range(self.n)], np.uint64)
        self.first = np.array([table[k].first for k in range(self.n)], np.uint64)
        self.boxes = np.array([[getattr(table[k].box, f) for f in ("x0", "y0", "z0", "x1", "y1", "z1")] for k in range(self.n)], np.uint32).reshape(self.n, 6)
        self.n_foreground = int(n_foreground)
        self.labels = labels

    def largest(self, k: int = 1) -> np.ndarray:
        """The ids of the min(k, n) largest components: by size descending, then by first voxel -- KEEP_LARGEST's order."""
        order = np.lexsort((np.arange(self.n), -self.sizes.astype(np.int64)))
        return (order[:max(int(k), 0)] + 1).astype(np.int64)

    def __len__(self):
        return self.n

    def __repr__(self):
        return "Components(n=%d, n_foreground=%d)" % (self.n, self.n_foreground)
