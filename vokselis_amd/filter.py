"""The weights and the request of the volume filter pass (vk_volume_filter, vk_filter_gaussian): Context.filter_volume, smooth_volume and
median_volume are built on these.  The arithmetic is the library's: gaussian_weights calls vk_filter_gaussian."""
import ctypes as C
import math

import numpy as np

from . import _native as N


def gaussian_weights(sigma: float, radius=None) -> np.ndarray:
    """vk_filter_gaussian: the 2 radius + 1 normalised weights of a Gaussian of `sigma` voxels as float32; radius None: min(6, ceil(3 sigma))."""
    sigma = float(sigma)
    if radius is None:
        if not (math.isfinite(sigma) and sigma > 0.0):
            raise ValueError("gaussian_weights: sigma must be finite and > 0")
        radius = min(N.FILTER_MAX_RADIUS, max(1, int(math.ceil(3.0 * sigma))))
    radius = int(radius)
    if radius < 0:
        raise ValueError("gaussian_weights: radius must be in [1, FILTER_MAX_RADIUS]")
    w = np.zeros(2 * min(radius, N.FILTER_MAX_RADIUS) + 1, np.float32)
    N.check(None, N.lib().vk_filter_gaussian(sigma, radius, w.ctypes.data_as(C.POINTER(C.c_float))))
    return w


def filter_request(weights=None, op: str = "convolve", install: bool = True) -> N.VkVolumeFilter:
    """A VkVolumeFilter from per-axis weights (wx, wy, wz): each None (radius 0: the axis is skipped) or an odd number 2 r + 1 of
    weights, r <= FILTER_MAX_RADIUS.  op: "convolve" or "median3" (weights are ignored).  Raises ValueError."""
    ops = {"convolve": N.FILTER_CONVOLVE, "median3": N.FILTER_MEDIAN3}
    if op not in ops:
        raise ValueError('op: "convolve" or "median3"')
    req = N.VkVolumeFilter()
    req.op = ops[op]
    req.flags = N.FILTER_INSTALL if install else 0
    if op == "convolve":
        if weights is None:
            weights = (None, None, None)
        if len(weights) != 3:
            raise ValueError("weights: (wx, wy, wz), each None or 2 r + 1 weights")
        for a, w in enumerate(weights):
            if w is None:
                continue
            w = np.asarray(w, np.float32).ravel()
            if len(w) % 2 == 0 or len(w) < 3 or len(w) > 2 * N.FILTER_MAX_RADIUS + 1:
                raise ValueError("weights: an odd number 2 r + 1 of weights per axis, 1 <= r <= FILTER_MAX_RADIUS (None: the axis is skipped)")
            req.radius[a] = len(w) // 2
            for k, v in enumerate(w):
                req.weights[a][k] = float(v)
    return req
