"""The request and the result of the measuring pass (vk_measure_components): Context.measure_components is built on these.  The library
returns one exact integer record per region; everything a user reads -- centroid, covariance, principal axes, mean, deviation, volume,
surface -- is derived here from those integers in Python's exact integer arithmetic and rounded once, by the final division."""
import math

import numpy as np

from . import _native as N

_FIELDS = [("n_voxels", "<u8"), ("first", "<u8"), ("box", "<u4", (6,)), ("sums", "<u8", (9,)), ("n_nonfinite", "<u8"), ("q_min", "<i8"), ("q_max", "<i8"),
           ("sum_q_hi", "<i8"), ("sum_q_lo", "<u8"), ("sum_qq_hi", "<u8"), ("sum_qq_lo", "<u8"), ("faces", "<u8", (3,))]
REGION_DTYPE = np.dtype(_FIELDS)
assert REGION_DTYPE.itemsize == 192


def measure_request(lo=0.0, hi=float("inf"), connectivity: int = 6, box=None, max_label=None) -> N.VkMeasureRequest:
    """A VkMeasureRequest.  max_label None: the library labels the range [lo, hi] under `connectivity` itself (box: None, "clip" or a
    voxel box).  max_label k >= 1: the caller brings the labels; the regions are 1 .. k, and range, connectivity and box must be left alone.
    Raises ValueError for what cannot be put into the struct; the library refuses the rest."""
    req = N.VkMeasureRequest()
    if max_label is None:
        req.lo, req.hi, req.connectivity = float(lo), float(hi), int(connectivity)
        req.flags = N.MEASURE_CLIP_BOX if box == "clip" else 0
    else:
        if int(max_label) != max_label or not 1 <= int(max_label) <= 0xFFFFFFFE:
            raise ValueError("max_label: an integer 1 .. 2^32 - 2")
        if box is not None:
            raise ValueError("box: labels cover the whole volume")
        req.max_label = int(max_label)
    return req


def _ratio(num: int, den: int) -> float:
    """num / den rounded once (Python's int / int is correctly rounded); NaN where the quotient has no meaning."""
    return num / den if den else math.nan


class Measurements:
    """The regions of Context.measure_components in id order (id k + 1 at index k).  Raw, all integers: n, n_regions, n_foreground, scale,
    dims (nx, ny, nz), sizes, first, boxes [n, 6], sums [n, 9] (x, y, z, xx, yy, zz, xy, xz, yz), n_nonfinite, q_min, q_max, sum_q and
    sum_qq (object arrays of Python ints: the 128-bit fields joined), faces [n, 3].  Derived: see the methods.  An empty region (an id no
    voxel carries) gives NaN wherever a quotient has no meaning."""

    def __init__(self, table, n: int, res: N.VkMeasureResult, dims):
        self.n = int(n)
        self.n_regions, self.n_foreground, self.scale = int(res.n_regions), int(res.n_foreground), int(res.scale)
        self.dims = tuple(int(d) for d in dims)
        rec = np.frombuffer(table, REGION_DTYPE, count=self.n).copy() if self.n else np.zeros(0, REGION_DTYPE)
        self.records = rec
        self.sizes, self.first, self.boxes, self.sums = rec["n_voxels"], rec["first"], rec["box"], rec["sums"]
        self.n_nonfinite, self.q_min, self.q_max, self.faces = rec["n_nonfinite"], rec["q_min"], rec["q_max"], rec["faces"]
        self.sum_q = np.array([(int(h) << 64) + int(l) for h, l in zip(rec["sum_q_hi"], rec["sum_q_lo"])] + [None], object)[:-1]
        self.sum_qq = np.array([(int(h) << 64) + int(l) for h, l in zip(rec["sum_qq_hi"], rec["sum_qq_lo"])] + [None], object)[:-1]

    def __len__(self):
        return self.n

    def __repr__(self):
        return "Measurements(n=%d, n_foreground=%d, scale=%d)" % (self.n, self.n_foreground, self.scale)

    def largest(self, k: int = 1) -> np.ndarray:
        """The ids of the min(k, n) largest regions: by size descending, then by id."""
        order = np.lexsort((np.arange(self.n), -self.sizes.astype(np.int64)))
        return (order[:max(int(k), 0)] + 1).astype(np.int64)

    # -- geometry
    @property
    def centroid(self) -> np.ndarray:
        """[n, 3]: the mean voxel index (x, y, z)."""
        return np.array([[_ratio(int(s), int(m)) for s in row[:3]] for m, row in zip(self.sizes, self.sums)], np.float64).reshape(self.n, 3)

    @property
    def centroid_unit(self) -> np.ndarray:
        """[n, 3]: (centroid + 0.5) / dims -- the unit-cube convention of the mesh and of Hit.pos."""
        return (self.centroid + 0.5) / np.array(self.dims, np.float64)

    def covariance(self, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
        """[n, 3, 3]: the covariance of the voxel positions (population form, divisor n) in the units of `spacing` = (sx, sy, sz): each
        entry is (n S_ab - S_a S_b) / n^2 from the exact integers, rounded once, then scaled by s_a s_b."""
        sp = np.array([float(s) for s in spacing], np.float64)
        pair = {(0, 0): 3, (1, 1): 4, (2, 2): 5, (0, 1): 6, (0, 2): 7, (1, 2): 8}
        out = np.full((self.n, 3, 3), math.nan)
        for k in range(self.n):
            m, s = int(self.sizes[k]), [int(v) for v in self.sums[k]]
            for (a, b), w in pair.items():
                out[k, a, b] = out[k, b, a] = _ratio(m * s[w] - s[a] * s[b], m * m) * sp[a] * sp[b]
        return out

    def principal_axes(self, spacing=(1.0, 1.0, 1.0)):
        """(values [n, 3], vectors [n, 3, 3]): the covariance's eigenvalues in descending order and their unit eigenvectors,
        vectors[k, :, j] belonging to values[k, j] (numpy.linalg.eigh).  NaN for an empty region."""
        cov = self.covariance(spacing)
        values, vectors = np.full((self.n, 3), math.nan), np.full((self.n, 3, 3), math.nan)
        for k in range(self.n):
            if np.isfinite(cov[k]).all():
                w, v = np.linalg.eigh(cov[k])
                values[k], vectors[k] = w[::-1], v[:, ::-1]
        return values, vectors

    def principal_lengths(self, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
        """[n, 3]: the full axes, longest first, of the uniform ellipsoid that has the region's covariance: 2 sqrt(5 lambda)."""
        values, _ = self.principal_axes(spacing)
        return 2.0 * np.sqrt(5.0 * np.maximum(values, 0.0))

    def volume(self, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
        return self.sizes.astype(np.float64) * float(spacing[0]) * float(spacing[1]) * float(spacing[2])

    def equivalent_diameter(self, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
        """The diameter of the ball of the region's volume."""
        return np.cbrt(6.0 * self.volume(spacing) / math.pi)

    def surface_area(self, spacing=(1.0, 1.0, 1.0)) -> np.ndarray:
        """The area of the region's exposed voxel faces, faces . (sy sz, sx sz, sx sy): the surface of the voxel staircase, an overestimate
        for a smooth shape (a large ball: by a factor of 1.5)."""
        sx, sy, sz = (float(s) for s in spacing)
        return self.faces.astype(np.float64) @ np.array([sy * sz, sx * sz, sx * sy])

    @property
    def touches_border(self) -> np.ndarray:
        """Whether a region's box reaches a face of the volume."""
        b, d = self.boxes.astype(np.int64).reshape(self.n, 6), np.array(self.dims, np.int64)
        return (self.sizes > 0) & ((b[:, :3] == 0).any(axis=1) | (b[:, 3:] == d).any(axis=1))

    # -- intensity, in sample values (q / scale), over the finite voxels
    @property
    def n_finite(self) -> np.ndarray:
        return self.sizes - self.n_nonfinite

    @property
    def mean(self) -> np.ndarray:
        return np.array([_ratio(int(s), int(m) * self.scale) for s, m in zip(self.sum_q, self.n_finite)], np.float64)

    @property
    def variance(self) -> np.ndarray:
        """(m sum q^2 - (sum q)^2) / (m scale)^2 over the m finite voxels, in exact integers, rounded once (population form)."""
        return np.array([_ratio(int(m) * int(qq) - int(q) * int(q), (int(m) * self.scale) ** 2) for q, qq, m in zip(self.sum_q, self.sum_qq, self.n_finite)], np.float64)

    @property
    def std(self) -> np.ndarray:
        return np.sqrt(self.variance)

    @property
    def min(self) -> np.ndarray:
        return np.where(self.n_finite > 0, self.q_min.astype(np.float64) / self.scale, math.nan)

    @property
    def max(self) -> np.ndarray:
        return np.where(self.n_finite > 0, self.q_max.astype(np.float64) / self.scale, math.nan)

    CSV_HEADER = ("id,n_voxels,first,x0,y0,z0,x1,y1,z1,cx,cy,cz,volume,equivalent_diameter,length_1,length_2,length_3,mean,std,min,max,n_nonfinite,"
                  "faces_x,faces_y,faces_z,surface_area,touches_border")

    def to_csv(self, path, spacing=(1.0, 1.0, 1.0)):
        """One line per region under CSV_HEADER; lengths, volume and area in the units of `spacing`."""
        c, vol, dia, lens, area = self.centroid, self.volume(spacing), self.equivalent_diameter(spacing), self.principal_lengths(spacing), self.surface_area(spacing)
        mean, std, lo, hi, border = self.mean, self.std, self.min, self.max, self.touches_border
        with open(path, "w") as f:
            f.write(self.CSV_HEADER + "\n")
            for k in range(self.n):
                cells = [k + 1, int(self.sizes[k]), int(self.first[k])] + [int(v) for v in self.boxes[k]]
                cells += ["%.17g" % v for v in (*c[k], vol[k], dia[k], *lens[k], mean[k], std[k], lo[k], hi[k])]
                cells += [int(self.n_nonfinite[k])] + [int(v) for v in self.faces[k]] + ["%.17g" % area[k], int(border[k])]
                f.write(",".join(str(v) for v in cells) + "\n")
