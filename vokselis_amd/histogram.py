"""The result of Context.volume_histogram (vk_volume_histogram): the counts of the stored texels over a domain, the categories outside it,
and the statistics of the region in sample values -- the units of set_transfer_function's domain and of an isovalue."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as N


class Histogram:
    """counts: uint64 [bins]; edges: float64 [bins + 1] over the domain; n_voxels = n_nan + n_below + n_above + counts.sum();
    min / max / mean / std in sample values (the kernel's scale divided out; std is the population deviation from the f64 sums over the
    finite texels, NaN without one); stats: the raw VkVolumeStats on the kernel's scale."""

    def __init__(self, counts: np.ndarray, domain, stats: N.VkVolumeStats):
        self.counts = np.asarray(counts, np.uint64)
        self.domain = (float(domain[0]), float(domain[1]))
        self.bins = int(self.counts.shape[0])
        self.edges = self.domain[0] + (self.domain[1] - self.domain[0]) * np.arange(self.bins + 1, dtype=np.float64) / max(self.bins, 1)
        self.stats = stats
        self.n_voxels, self.n_nan, self.n_below, self.n_above, self.n_finite = (int(stats.n_voxels), int(stats.n_nan), int(stats.n_below),
                                                                                int(stats.n_above), int(stats.n_finite))
        self.scale = float(stats.scale)
        self.min = float(stats.min) / self.scale
        self.max = float(stats.max) / self.scale
        if self.n_finite:
            m = float(stats.sum) / self.n_finite
            var = max(float(stats.sum_sq) / self.n_finite - m * m, 0.0)
            self.mean, self.std = m / self.scale, math.sqrt(var) / self.scale
        else:
            self.mean = self.std = float("nan")

    def window(self, p_lo: float = 0.01, p_hi: float = 0.99):
        """vk_histogram_window: the (lo, hi) of the bins that hold the percentiles p_lo .. p_hi of the counted texels -- a domain for
        set_transfer_function."""
        lo, hi = C.c_float(), C.c_float()
        c = np.ascontiguousarray(self.counts, np.uint64)
        N.check(None, N.lib().vk_histogram_window(c.ctypes.data_as(C.POINTER(C.c_uint64)), self.bins, self.domain[0], self.domain[1], float(p_lo), float(p_hi),
                                                  C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def __repr__(self):
        return (f"Histogram(bins={self.bins}, domain={self.domain}, n_voxels={self.n_voxels}, n_nan={self.n_nan}, n_below={self.n_below}, "
                f"n_above={self.n_above}, min={self.min:.6g}, max={self.max:.6g}, mean={self.mean:.6g}, std={self.std:.6g})")
