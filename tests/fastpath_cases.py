"""The cases that sit at, near and beyond the three limits of the rule which sends a cell march down its unclamped build
(vk_hostmath.hpp: cell_march_fast), shared by tests/test_fastpath_cpu.py (the references alone, and the replay audit of
tests/fastpath_fuzz.cpp) and tests/test_fastpath_gpu.py (the kernels).

Every case is small -- an image of 32 x 16 or less, a volume under 100 KB -- and long: volumes of up to 4080 voxels along one axis seen
down that axis, steps down to a twentieth of a voxel (80 000 trips per ray), cameras out to a thousand units through a field of view
narrowed to the box.  The volumes are mostly exactly transparent with a few faint slabs, so rays run their full length; the first and
the last brick along the long axis are faint, different from each other and from zero, so a lookup that lands on the wrong end shows.

`rule_fast` is this module's own statement of the rule, in Python floats, written from the derivation and not from the header; the CPU
module holds it to the header's through the audit program, the GPU module holds vk_debug_march_path to it."""
from __future__ import annotations

import functools
import math
import dataclasses
from dataclasses import dataclass

import numpy as np

PI = math.pi
CENTRE = (0.5, 0.5, 0.5)
LUT_BUDGET = 16384
TRIPS_NUMPY = 5000  # the numpy references join in on cases of at most this many trips per ray

# the seven rows: 16 x 8 frames of camera_blob(dist, 0.02, pi/2 + 0.01, centre, 2.0) down the long x axis of an nx x 4 x 4 volume -- (nx, dist,
# dt_scale, the largest x index that a rule which looks at the camera's distance alone lets the unclamped build look up; the table ends at nx)
ROWS = ((2048, 3.4, 0.25, 2049), (2048, 3.4, 0.05, 2056), (4000, 3.4, 0.25, 4004), (4000, 2.0, 0.1, 4002), (4000, 3.4, 0.1, 4011),
        (4000, 2.0, 0.05, 4018), (4000, 3.4, 0.05, 4035))


@dataclass
class Case:
    name: str
    dims: tuple          # (nx, ny, nz)
    cam: tuple           # arguments of oracle.camera_blob
    k: float             # the field of view's scale (narrow_blob): 1 is the stock field
    W: int
    H: int
    dt: float
    f16: bool = False
    tags: tuple = ()
    u16: bool = False    # an R16_UNORM volume: the u8 values times 257, the same normalised values

    @property
    def kind(self):
        return 'f16' if self.f16 else ('u16' if self.u16 else 'u8')

    @property
    def cell_bytes(self):
        """Of the PACKED layout; PACKED_PAIRS (u8 only) has 16."""
        return 8 if self.kind == 'u8' else 16

    @property
    def long_axis(self):
        return int(np.argmax(self.dims))

    def blob(self, O):
        return narrow_blob(O, self.cam, self.k)

    @functools.cached_property
    def vol(self):
        v = volume(self.dims, self.f16)
        return v.astype(np.uint16) * np.uint16(257) if self.u16 else v

    def __repr__(self):
        return f"Case({self.name}: dims={self.dims} {self.kind} {self.W}x{self.H} dt={self.dt} cam={self.cam} k={self.k})"


# ---- cameras ----

def narrow_blob(O, cam, k=1.0):
    """O.camera_blob(*cam) with the field of view scaled by k (a power of two, so that the scaling is exact): NDC x and y reach k times as
    far -- columns 0 and 1 of inv_proj times k, rows 0 and 1 of proj_view by 1 / k, the eye as it is.  At k = 1 the stock blob, bit for
    bit.  A thousand units out the stock field puts the unit box under one pixel."""
    b = np.frombuffer(O.camera_blob(*cam), np.float32).copy()
    assert b.size == 36 and k > 0 and math.frexp(k)[0] == 0.5
    kk = np.float32(k)
    b[20:28] *= kk                                  # inv_proj, column-major: columns 0 and 1
    pv = b[4:20].reshape(4, 4)                      # proj_view [column][row]
    pv[:, 0:2] /= kk
    return b.tobytes()


def eye_of(O, c):
    return np.frombuffer(c.blob(O), np.float32)[:3].copy()


def down_axis(axis, dist, aspect=2.0):
    """The view down `axis` from `dist` away, a hundredth of a radian off the axis (axis 0: the rows' camera)."""
    if axis == 0:
        return (dist, 0.02, PI / 2 + 0.01, CENTRE, aspect)
    if axis == 2:
        return (dist, 0.02, 0.01, CENTRE, aspect)
    return (dist, PI / 2 - 0.02, 0.3, CENTRE, aspect)


def field_for(dist):
    k = 1.0
    while k * dist > 1.5:
        k *= 0.5
    return k


# ---- the rule, restated ----

def _ulp32(x):
    x = np.float32(x)
    return float(np.nextafter(x, np.float32(np.inf)) - x)


def reach_of(eye):
    e = np.asarray(eye, np.float32)
    return np.float32(np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2], dtype=np.float32) + np.float32(4.0))


def cell_array_bytes(dims, cell_bytes):
    nb = [((n - 1) >> 2) + 2 for n in dims]
    return nb[0] * nb[1] * nb[2] * 64 * cell_bytes


def rule_fast(dims, eye, dt, cell_bytes=8, safe_flag=False):
    """Whether a NAIVE_TRILINEAR march of a cell layout may run unclamped.  Three limbs -- offsets in 32 bits, the index tables within
    their LDS budget, and f32 drift below the quarter cell the tables have to spare next to the probe-ahead step: the set-up's 64 ulp of
    the reach, and per trip half an ulp of the reach on t and half an ulp of 2 on p, over max(dims) / dt_scale trips and the slack of a
    loop variable that is itself drifting (a sixteenth at the most, where the render is accepted at all: dt >= 8 ulp)."""
    nmax = float(max(dims))
    reach = reach_of(eye)
    u = _ulp32(reach)
    if safe_flag or cell_array_bytes(dims, cell_bytes) - cell_bytes + 16 >= 2 ** 32:
        return False
    if ((sum(dims) + 9 + 3) & ~3) * 4 > LUT_BUDGET:
        return False
    if not (dt / nmax >= 8.0 * u):
        return False
    trips = 1.125 * nmax / dt + 4.0
    return nmax * (64.0 * u + trips * (0.5 * u + 0.5 * _ulp32(2.0))) < 0.25


def render_accepted(dims, eye, dt):
    """check_render's guard: dt_scale / max(dims) >= 8 ulp(reach), in f32."""
    return bool(np.float32(dt) / np.float32(max(dims)) >= np.float32(8.0) * np.float32(_ulp32(reach_of(eye))))


def precision_edge(dims, dt):
    """The reach (a power of two: the rule's ulp doubles there) from which on the rule says "safe" for these dims and dt_scale; None when
    it says so at every distance."""
    if not rule_fast(dims, (0.0, 0.0, 0.0), dt):
        return None
    e = 8.0
    while rule_fast(dims, (e - 4.0, 0.0, 0.0), dt):
        e *= 2.0
    return e


# ---- volumes ----

def volume(dims, f16=False):
    """Exactly transparent (10 of 255: the built-in transfer and the tables of table() give alpha 0 below a tenth) but for: the first brick
    along the long axis at 27, the last at 29, and slabs of 26 .. 30 at five places along it -- all just above the tenth, faint enough that
    80 000 samples through them stay under the early-out's 0.95."""
    nx, ny, nz = dims
    ax = int(np.argmax(dims))
    n = dims[ax]
    line = np.full(n, 10, np.uint8)
    line[:min(4, n)] = 27
    line[-min(4, n):] = 29
    for j, at in enumerate((0.17, 0.38, 0.5, 0.71, 0.9)):
        a = int(at * n)
        line[a:a + max(2 if n >= 64 else 1, n // 200)] = 26 + j
    shape = [1, 1, 1]
    shape[2 - ax] = n
    vol = np.broadcast_to(line.reshape(shape), (nz, ny, nx)).copy()
    if f16:
        return (vol.astype(np.float32) / np.float32(255.0)).astype(np.float16)
    return vol


def table(n=64):
    """Alpha exactly 0 below a tenth of the domain, then faint; colours that tell the values apart."""
    x = np.arange(n) / (n - 1)
    t = np.empty((n, 4), np.float32)
    t[:, 0], t[:, 1], t[:, 2] = 0.2 + 0.8 * x, 0.9 - 0.6 * x, 0.5 + 0.5 * np.sin(40.0 * x)
    t[:, 3] = np.where(x < 0.1, 0.0, 0.0002 + 0.002 * (x - 0.1))
    return t


DOMAIN = (0.0, 1.0)


# ---- the list ----

@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # 1. the seven rows
    for nx, dist, dt, _ in ROWS:
        out.append(Case(f"row {nx}x4x4 from {dist} at dt {dt}", (nx, 4, 4), down_axis(0, dist), 1.0, 16, 8, dt, tags=("row",)))
    # 2. the long axis in x, y and z at three step sizes, through a quarter of the stock field: most rays run the whole length
    for dims in ((2048, 4, 4), (4, 4075, 4), (4, 4, 4079)):
        for j, dt in enumerate((1.0, 0.25, 0.05)):
            ax = int(np.argmax(dims))
            out.append(Case(f"long {'xyz'[ax]} {'x'.join(map(str, dims))} at dt {dt}", dims, down_axis(ax, 2.6), 0.25, 16, 8, dt, f16=(j == 1 and ax == 0),
                            tags=("long",)))
    # 3. the tables' budget: 4079 + 4 + 4 fits 16 KB, 4080 + 4 + 4 does not
    for nx in (4079, 4080):
        out.append(Case(f"budget {nx}x4x4", (nx, 4, 4), down_axis(0, 2.2), 1.0, 16, 8, 1.0, tags=("budget",)))
    # 4. the eye just inside and just outside the precision limit.  2048 x 4 x 4 has none any more (its rays are too long at every
    # distance): it keeps the limit of the distance-only rule, |eye| + 4 = 16.
    for dims, dt, aspect in (((32, 32, 32), 1.0, 1.0), ((256, 8, 8), 1.0, 2.0), ((2048, 4, 4), 1.0, 2.0)):
        edge = precision_edge(dims, dt) or 16.0
        for side, off in (("inside", -0.75), ("outside", 0.75)):
            dist = edge - 4.0 + off * min(1.0, edge / 32.0) * 4.0
            ax = int(np.argmax(dims))
            cam = down_axis(ax, dist, aspect) if dims[0] != dims[1] else (dist, 0.4, 0.7, CENTRE, aspect)
            out.append(Case(f"eye {side} {'x'.join(map(str, dims))} at {dist:g}", dims, cam, field_for(dist), 32 if aspect == 2.0 else 16, 16, dt,
                            tags=("eye", side)))
    # 5. long rays the rule still sends down the unclamped build: each is under the drift limit by its dims and dt_scale together, and the
    # ones marked "over" are the same views one notch past it
    for name, dims, dt, f16 in (("512 at 1", (512, 4, 4), 1.0, False), ("700 at 1", (4, 700, 4), 1.0, False), ("256 at .25", (4, 4, 256), 0.25, False),
                                ("128 at .05", (128, 4, 4), 0.05, False), ("1024 at 4", (1024, 4, 4), 4.0, False), ("640 at 1.25", (640, 5, 3), 1.25, False),
                                ("600 at 1 f16", (600, 4, 4), 1.0, True), ("300 at .25", (4, 300, 6), 0.25, False), ("96 at .05 f16", (5, 4, 96), 0.05, True),
                                ("720 at 1", (720, 4, 4), 1.0, False), ("400 at .5", (400, 7, 9), 0.5, False)):
        ax = int(np.argmax(dims))
        out.append(Case("fast " + name, dims, down_axis(ax, 1.9), 1.0, 16, 8, dt, f16=f16, tags=("fast",)))
    for name, dims, dt in (("840 at 1", (840, 4, 4), 1.0), ("180 at .05", (180, 4, 4), 0.05)):
        out.append(Case("over " + name, dims, down_axis(0, 1.9), 1.0, 16, 8, dt, tags=("over",)))
    # 6. R16_UNORM volumes, whose kernels are units of their own: a row, a long ray the rule keeps unclamped, and an eye pair
    by = {c.name: c for c in out}
    for name in ("row 2048x4x4 from 3.4 at dt 0.25", "fast 512 at 1"):
        out.append(dataclasses.replace(by[name], name="u16 " + name, u16=True))
    for c in [c for c in out if c.name.startswith(("eye inside 256x8x8", "eye outside 256x8x8"))]:
        out.append(dataclasses.replace(c, name="u16 " + c.name, u16=True))
    return tuple(out)


N_CASES = 7 + 9 + 2 + 6 + 11 + 2 + 4

# the other families run on a long-axis case and a far-camera case on EACH side of the rule -- the unclamped loops of every family at
# their limits, and the clamped ones beyond -- and on the long u16 ray the rule keeps unclamped
FAMILY_CASES = ("fast 720 at 1", "long x 2048x4x4 at dt 0.25", "eye inside 32x32x32", "eye outside 32x32x32", "u16 fast 512 at 1")


def family_cases():
    out = [c for c in cases() if any(c.name.startswith(p) for p in FAMILY_CASES)]
    assert len(out) == len(FAMILY_CASES), out
    return out


def batch_cameras(O):
    """Five cameras on the 32^3 volume, the fourth beyond the precision limit: (blobs, index of the far one, W, H)."""
    edge = precision_edge((32, 32, 32), 1.0)
    far = edge - 4.0 + 3.0
    cams = [((1.1, 0.3, 0.4, CENTRE, 2.0), 1.0), ((1.4, -0.5, 2.0, CENTRE, 2.0), 1.0), ((0.8, 0.1, 4.1, CENTRE, 2.0), 1.0),
            ((far, 0.4, 0.7, CENTRE, 2.0), field_for(far)), ((2.3, 0.9, 5.2, CENTRE, 2.0), 1.0)]
    return [narrow_blob(O, c, k) for c, k in cams], 3, 32, 16
