"""Planes for the slice pass (Context.render_slice; vk_render_slice): `Slice` builds the four vectors of a VkSlice in double and rounds
each component once to f32.

Coordinates are the unit cube's: axis c of the volume runs over [0, 1] whatever its voxel count and spacing.  `dims` (nx, ny, nz) and
`spacing` give the volume's physical shape; lengths (`extent`, `thickness`) are in units of its longest physical side, so that on a cubic
volume they are unit-cube lengths, and pixels come out square in physical space."""
from __future__ import annotations

import math

from . import _native as N

_REDUCE = {"max": N.SLAB_MAX, "min": N.SLAB_MIN, "mean": N.SLAB_MEAN}


def _reduce(reduce) -> int:
    if isinstance(reduce, str):
        if reduce not in _REDUCE:
            raise ValueError("reduce: 'max', 'min' or 'mean'")
        return _REDUCE[reduce]
    if int(reduce) not in _REDUCE.values():
        raise ValueError("reduce: SLAB_MAX, SLAB_MIN or SLAB_MEAN")
    return int(reduce)


def _make(origin, du, dv, dn, samples, reduce) -> N.VkSlice:
    samples = int(samples)
    if not 1 <= samples <= N.SLICE_MAX_SAMPLES:
        raise ValueError("samples must be in [1, %d]" % N.SLICE_MAX_SAMPLES)
    s = N.VkSlice()
    for name, v in (("origin", origin), ("du", du), ("dv", dv), ("dn", dn)):
        v = tuple(float(x) for x in v)
        if len(v) != 3:
            raise ValueError(name + " needs three components")
        if not all(math.isfinite(x) and abs(x) <= N.SLICE_MAX_COORD for x in v):
            raise ValueError(name + ": a component is not finite or beyond +-SLICE_MAX_COORD")
        for i in range(3):
            getattr(s, name)[i] = v[i]  # the one rounding to f32
    s.samples = samples
    s.reduce = _reduce(reduce)
    return s


def _unit(v, what):
    n = math.sqrt(sum(x * x for x in v))
    if not (n > 0.0 and math.isfinite(n)):
        raise ValueError(what + " has no direction")
    return tuple(x / n for x in v)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


class Slice:
    """Builders of VkSlice.  Every method returns a VkSlice ready for Context.render_slice / slice_probe."""

    @staticmethod
    def raw(origin, du, dv, dn=(0.0, 0.0, 0.0), samples=1, reduce="max") -> N.VkSlice:
        """The four vectors as given (unit-cube coordinates), checked against vk_render_slice's bounds."""
        return _make(origin, du, dv, dn, samples, reduce)

    @staticmethod
    def plane(centre, normal, up, width, height, extent, thickness=0.0, samples=1, reduce="max", spacing=(1.0, 1.0, 1.0), dims=None) -> N.VkSlice:
        """The plane through `centre` (unit-cube coordinates) with `normal` pointing at the viewer and `up` towards the top of the image (both
        directions in physical space; `up` need not be perpendicular to `normal`), seen in a width x height pixel frame whose width covers
        `extent`.  +x on screen is up x normal, +y on screen (down) is -up.  A slab of `samples` planes spans `thickness` along the normal,
        centred on the plane.  Without `dims` the volume is taken as a cube of equal spacing."""
        width, height, samples = int(width), int(height), int(samples)
        if width < 1 or height < 1:
            raise ValueError("width and height must be at least 1")
        if not (float(extent) > 0.0 and math.isfinite(float(extent))):
            raise ValueError("extent must be finite and > 0")
        dims = (1, 1, 1) if dims is None else tuple(int(d) for d in dims)
        side = tuple(float(d) * float(sp) for d, sp in zip(dims, spacing))
        if len(side) != 3 or not all(s > 0.0 and math.isfinite(s) for s in side):
            raise ValueError("dims and spacing need three positive components")
        longest = max(side)
        size = tuple(s / longest for s in side)  # the physical side per axis, the longest 1
        n = _unit(normal, "normal")
        d = sum(a * b for a, b in zip(up, n))
        upp = _unit(tuple(a - d * b for a, b in zip(up, n)), "up (parallel to normal)")
        right = _cross(upp, n)
        px = float(extent) / width  # a pixel's physical side
        du = tuple(right[i] * px / size[i] for i in range(3))
        dv = tuple(0.0 - upp[i] * px / size[i] for i in range(3))  # (0 - x: a zero component is +0)
        step = float(thickness) / (samples - 1) if samples > 1 else 0.0
        dn = tuple(n[i] * step / size[i] for i in range(3))
        origin = tuple(float(centre[i]) - 0.5 * (width - 1) * du[i] - 0.5 * (height - 1) * dv[i] for i in range(3))
        return _make(origin, du, dv, dn, samples, reduce)

    @staticmethod
    def _ortho(axis, dims, index, width, height, samples, reduce):
        nx, ny, nz = (int(d) for d in dims)
        n = (nx, ny, nz)
        a, b = {2: (0, 1), 1: (0, 2), 0: (1, 2)}[axis]  # the screen's x and y axes
        du, dv, dn, origin = [0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3
        du[a] = 1.0 / int(width)
        dv[b] = 1.0 / int(height)
        dn[axis] = 1.0 / n[axis]
        origin[a], origin[b], origin[axis] = 0.5 / int(width), 0.5 / int(height), (float(index) + 0.5) / n[axis]
        return _make(origin, du, dv, dn, samples, reduce)

    @staticmethod
    def axial(dims, index, width, height, samples=1, reduce="max") -> N.VkSlice:
        """The z = index plane of voxel centres: pixel (px, py) is voxel (x, y) = (px, py) where width x height is nx x ny -- pixel centres
        on texel centres.  A slab takes `samples` neighbouring planes, one voxel apart, centred on `index`."""
        return Slice._ortho(2, dims, index, width, height, samples, reduce)

    @staticmethod
    def coronal(dims, index, width, height, samples=1, reduce="max") -> N.VkSlice:
        """The y = index plane: pixel (px, py) is voxel (x, z) = (px, py) where width x height is nx x nz."""
        return Slice._ortho(1, dims, index, width, height, samples, reduce)

    @staticmethod
    def sagittal(dims, index, width, height, samples=1, reduce="max") -> N.VkSlice:
        """The x = index plane: pixel (px, py) is voxel (y, z) = (px, py) where width x height is ny x nz."""
        return Slice._ortho(0, dims, index, width, height, samples, reduce)
