"""The request and the result of the geodesic-distance pass (vk_geodesic_distance), and the path from a voxel back to a source:
Context.geodesic_distance is built on these."""
import math

import numpy as np

from . import _native as N

FACES = {"x-": N.GEO_FACE_X0, "x+": N.GEO_FACE_X1, "y-": N.GEO_FACE_Y0, "y+": N.GEO_FACE_Y1, "z-": N.GEO_FACE_Z0, "z+": N.GEO_FACE_Z1}


def face_mask(faces) -> int:
    """The mask of a face name ("x-", "x+", "y-", "y+", "z-", "z+") or of several."""
    if isinstance(faces, str):
        faces = (faces,)
    mask = 0
    for f in faces:
        if f not in FACES:
            raise ValueError("a face is one of 'x-', 'x+', 'y-', 'y+', 'z-', 'z+'")
        mask |= FACES[f]
    return mask


def geodesic_request(lo, hi=float("inf"), sources=("x-",), seeds=(), targets=(), connectivity: int = 26, spacing=(1, 1, 1), gain: float = 0.0, fill_out: float = 0.0,
                     fill_unreached: float = 0.0, box=None, install: bool = True) -> N.VkGeodesicRequest:
    """A VkGeodesicRequest.  sources, targets: face names; seeds: up to GEO_MAX_SEEDS voxels (x, y, z); spacing: three integers
    1 .. DIST_MAX_SPACING (x, y, z); gain: 0 asks for the automatic gain (the farthest reached voxel stores full scale), else finite and
    > 0.  Raises ValueError for what cannot be put into the struct; the library refuses the rest."""
    spacing = tuple(spacing)
    if len(spacing) != 3 or any(int(s) != s or not 1 <= int(s) <= N.DIST_MAX_SPACING for s in spacing):
        raise ValueError("spacing: three integers 1 .. DIST_MAX_SPACING (x, y, z)")
    if connectivity not in (6, 18, 26):
        raise ValueError("connectivity: 6, 18 or 26")
    seeds = [tuple(s) for s in seeds]
    if len(seeds) > N.GEO_MAX_SEEDS or any(len(s) != 3 or any(int(v) != v or not 0 <= int(v) < 2 ** 32 for v in s) for s in seeds):
        raise ValueError("seeds: at most GEO_MAX_SEEDS voxels (x, y, z)")
    gain = float(gain)
    if not (math.isfinite(gain) and gain >= 0.0):
        raise ValueError("gain: 0 (automatic), or finite and > 0")
    req = N.VkGeodesicRequest()
    req.lo, req.hi, req.gain, req.fill_out, req.fill_unreached = float(lo), float(hi), gain, float(fill_out), float(fill_unreached)
    req.connectivity = int(connectivity)
    req.flags = (N.GEO_CLIP_BOX if isinstance(box, str) and box == "clip" else 0) | (N.GEO_INSTALL if install else 0)
    req.spacing[0], req.spacing[1], req.spacing[2] = (int(s) for s in spacing)
    req.source_faces, req.target_faces, req.n_seeds = face_mask(sources), face_mask(targets), len(seeds)
    for k, s in enumerate(seeds):
        req.seeds[k][0], req.seeds[k][1], req.seeds[k][2] = (int(v) for v in s)
    return req


class Geodesic:
    """The totals of Context.geodesic_distance -- n_foreground, n_sources, n_reached, n_saturated, n_target_reached, sum_g, max_g,
    target_min and the gain used -- and what derives from them: n_unreached, reached_fraction, percolates (a target voxel was reached),
    max_distance, mean_distance and target_distance in the units of the spacing (g / 256; target_distance is inf when nothing
    percolates), tortuosity(axis); where asked for, g (uint32 [nz, ny, nx], GEO_INF where unreached or off the set), distance (float64,
    inf there) and dense (the stored map [nz, ny, nx]).  spacing and extent (the box's extents x, y, z) are the request's."""

    def __init__(self, res: N.VkGeodesicResult, spacing=(1, 1, 1), extent=(1, 1, 1), g=None, dense=None):
        for name in ("n_foreground", "n_sources", "n_reached", "n_saturated", "n_target_reached", "sum_g", "max_g", "target_min"):
            setattr(self, name, int(getattr(res, name)))
        self.gain = float(res.gain)
        self.spacing, self.extent = tuple(int(s) for s in spacing), tuple(int(e) for e in extent)
        self.n_unreached = self.n_foreground - self.n_reached
        self.reached_fraction = self.n_reached / self.n_foreground if self.n_foreground else 0.0
        self.percolates = self.target_min != N.GEO_INF
        self.max_distance = self.max_g / N.GEO_UNIT
        self.mean_distance = self.sum_g / (N.GEO_UNIT * self.n_reached) if self.n_reached else 0.0
        self.target_distance = self.target_min / N.GEO_UNIT if self.percolates else math.inf
        self.g, self.dense = g, dense

    @property
    def distance(self):
        """g in the units of the spacing as float64, inf where g is GEO_INF (None without g)."""
        if self.g is None:
            return None
        d = self.g.astype(np.float64) / N.GEO_UNIT
        d[self.g == N.GEO_INF] = math.inf
        return d

    def tortuosity(self, axis) -> float:
        """target_min / (256 spacing[a] (extent_a - 1)): the way through over the straight way along axis a (0, 1, 2 or "x", "y", "z");
        inf when the set does not percolate.  Raises ValueError when the extent along the axis is 1."""
        a = "xyz".index(axis) if isinstance(axis, str) else int(axis)
        if self.extent[a] <= 1:
            raise ValueError("tortuosity: the extent along the axis is 1")
        if not self.percolates:
            return math.inf
        return self.target_min / (N.GEO_UNIT * self.spacing[a] * (self.extent[a] - 1))

    def __repr__(self):
        return "Geodesic(n_foreground=%d, n_sources=%d, n_reached=%d, max_distance=%.6g, target_distance=%.6g)" % (self.n_foreground, self.n_sources, self.n_reached, self.max_distance,
                                                                                                                   self.target_distance)


def step_cost(spacing, dx: int, dy: int, dz: int) -> int:
    """w(d): the largest r with r r <= 65536 sum_c (spacing[c] d_c)^2."""
    return math.isqrt(((spacing[0] * dx) ** 2 + (spacing[1] * dy) ** 2 + (spacing[2] * dz) ** 2) << 16)


def geodesic_path(g, voxel, spacing=(1, 1, 1), connectivity: int = 26):
    """The shortest path from `voxel` (x, y, z) back to a source through g (uint32 [nz, ny, nx]), on the host: from v to the adjacent u
    with g(u) + w == g(v), the smallest offset index (dx + 1 + 3 (dy + 1) + 9 (dz + 1)) on a tie, until g == 0.  Returns the voxels as
    an (n, 3) int64 array, `voxel` first.  Raises ValueError on an unreached voxel and on a saturated one (its g is no path's length)."""
    if connectivity not in (6, 18, 26):
        raise ValueError("connectivity: 6, 18 or 26")
    conn_sum = {6: 1, 18: 2, 26: 3}[connectivity]
    spacing = tuple(int(s) for s in spacing)
    nz, ny, nx = g.shape
    x, y, z = (int(v) for v in voxel)
    if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
        raise ValueError("geodesic_path: the voxel lies outside the array")
    here = int(g[z, y, x])
    if here == N.GEO_INF:
        raise ValueError("geodesic_path: the voxel is unreached")
    if here == N.GEO_FAR:
        raise ValueError("geodesic_path: the voxel is saturated")
    steps = []
    for o in range(27):
        dx, dy, dz = o % 3 - 1, o // 3 % 3 - 1, o // 9 - 1
        if 1 <= abs(dx) + abs(dy) + abs(dz) <= conn_sum:
            steps.append((dx, dy, dz, step_cost(spacing, dx, dy, dz)))
    path = [(x, y, z)]
    while here != 0:
        for dx, dy, dz, w in steps:
            ux, uy, uz = x + dx, y + dy, z + dz
            if 0 <= ux < nx and 0 <= uy < ny and 0 <= uz < nz and int(g[uz, uy, ux]) + w == here:
                x, y, z, here = ux, uy, uz, here - w
                break
        else:
            raise ValueError("geodesic_path: g is no geodesic distance under this spacing and connectivity")
        path.append((x, y, z))
    return np.array(path, np.int64).reshape(-1, 3)
