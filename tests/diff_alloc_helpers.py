"""What the allocation-failure sweep of vk_steady_diffusion (tests/test_diff_alloc_failure_gpu.py) needs beside
tests/alloc_failure_cases.py: a context with the 64 x 64 frame, the hook, and what a failed call must leave as it was."""
import ctypes as C

import numpy as np

from alloc_failure_cases import VK_OK, H, W


class Env:
    """The package and the outputs of the restatement, computed once each and left unchanged."""

    def __init__(self, V):
        self.V, self.N, self.lib = V, V.native, None
        self._expected = {}

    def expected(self, key, make):
        if key not in self._expected:
            e = make()
            for a in (e if isinstance(e, tuple) else (e,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._expected[key] = e
        return self._expected[key]


def new_ctx(E):
    V = E.V
    cam = V.Camera(1.0, 0.5, 1.0, (0.5, 0.5, 0.5), W / H)
    ctx = V.Context(W, H, cam, backbuffer=(W, H), out_format=V.OUT_RGBA32F)
    try:
        ctx.update()
    except BaseException:
        ctx.close()
        raise
    return ctx


def last_error(E, ctx):
    return E.N.lib().vk_last_error(ctx.handle).decode()


def arm(ctx, k):
    ctx.set_param("alloc_fail_at", k)


STATE = ("dims", "format", "layout", "device bytes", "empty fraction", "projection", "isosurface", "map grid", "skip maps", "frame")


def state(E, ctx):
    """vk_volume_info, vk_volume_empty_fraction, the projection, the isosurface, the skip maps' bytes and the frame."""
    N, L = E.N, E.N.lib()
    dims, fmt, lay, nbytes = (C.c_uint32 * 3)(), C.c_int(), C.c_int(), C.c_size_t()
    assert L.vk_volume_info(ctx.handle, dims, C.byref(fmt), C.byref(lay), C.byref(nbytes)) == VK_OK
    ef = C.c_double(-1.0)
    N.check(ctx.handle, L.vk_volume_empty_fraction(ctx.handle, C.byref(ef)))
    grid, maps = ctx.read_skip_maps()
    N.check(ctx.handle, L.vk_backbuffer_clear(ctx.handle))
    N.check(ctx.handle, L.vk_render(ctx.handle, N.MODE_NAIVE_TRILINEAR, 0, 0, W, H, 1.0, 0))
    return (tuple(dims), fmt.value, lay.value, nbytes.value, ef.value, ctx.projection, ctx.isosurface, grid, maps.tobytes(), ctx.read_backbuffer().tobytes())


def state_differences(a, b):
    return "" if a == b else ", ".join(n for n, x, y in zip(STATE, a, b) if x != y) + " changed"
