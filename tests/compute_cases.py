"""The seeded fuzz cases of the compute twin (VK_MODE_COMPUTE_NEAREST: raycast_compute.wgsl's render / get_col2), shared by
tests/test_compute_fuzz_cpu.py (the float64 numpy reference against the C oracle) and tests/test_compute_fuzz_gpu.py (the literal twin,
the records kernel and its skip policies against the oracle), so that both walk the same list.

Each case fixes the two rgba16f volumes (density: colour + opacity; normals: xyz + the unused w), the camera, the image and an optional
tile, dt_scale and whether RGBA16F output is checked.  Volume kinds, camera kinds and dt are dealt in cycles of coprime lengths (7, 5, 6);
the draw fills in their parameters.  The volumes carry the f16 edge patterns of tests/builtin_cases.py (+-0, subnormals, +-1, +-65504,
+-inf, NaN patterns) in the colour, the opacity and each normal component separately, opacities on both sides of the point where
smoothstep(0, 0.7, a^3) becomes 0, air of exactly-zero opacity with NaN normals (the xor example's holes), air whose colour or normal would
make a zero-weight step NaN, and the xor generator's own volumes.  Walk cases put a few small blobs in a volume of 128..256 voxels along the
ray, so that the records kernel walks hops of up to its 61-voxel skip radius; far cases put the eye 10..60 units away, and four put it
45, 150 and 300 units away down a 256-voxel axis at the smallest dt the library accepts there, where every t = t + dt rounds up by half an
ulp (1.4 %, 3 % and 6 % of dt): their walks must still end before the first record that can contribute.

A case is tagged `divergent` when a record's normal x or z is +-inf or NaN while its normal y is negative and the record can add to the
colour: there the records kernel's short form of the shade, max(0, -n.y), is not the text's NaN-laundered max(0, dot((0, -1, 0), n)) = 0
(vk_compute.hpp documents it), and only the records-vs-records equalities apply.  Every other case must give the literal twin's bits."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from builtin_cases import F16_EDGE_BITS, F16_NAN_BITS

SEED = 20261016
DTS = (0.013, 0.15, 0.5, 1.0, 1.7, 3.5)
N_RANDOM = 35
FIXED_DIMS = ((1, 1, 1), (2, 3, 5), (4, 4, 4), (5, 4, 9), (8, 8, 8), (3, 1, 17), (13, 7, 4))
EDGE_BITS = tuple(F16_EDGE_BITS.values())
# opacities whose smoothstep(0, 0.7, a^3) is exactly 0 (<= 0, NaN) and the smallest that are not (the subnormals: a^3 is a normal f32,
# s * s an f32 subnormal)
ZERO_OPACITY_BITS = (0x0000, 0x8000, 0x8001, 0xBC00, 0xFBFF, 0xFC00) + F16_NAN_BITS
TINY_OPACITY_BITS = (0x0001, 0x0002, 0x03FF, 0x0400, 0x1000)
NONFINITE_BITS = (0x7C00, 0xFC00) + F16_NAN_BITS


# dt / ulp(t) on the centre ray of the far cases that drift (dt = 0.01 dt_scale): a fraction of ~0.52 rounds every t = t + dt up
DRIFT_ULPS = {"far t~45 drift": 34.52, "far t~150 drift": 16.52, "slab at 115, eye 150": 16.52, "slab at 110, eye 300": 8.52}


@dataclass
class Case:
    name: str
    den: np.ndarray             # (nz, ny, nx, 4) f16: colour, opacity
    nrm: np.ndarray             # (nz, ny, nx, 4) f16: normal xyz, w unused
    cam: tuple                  # arguments of oracle.camera_blob: zoom, pitch, yaw, target, aspect
    kind: int                   # 0 orbit, 1 eye inside, 2 axis-aligned, 3 grazing a face, 4 far
    W: int
    H: int
    dt: float
    tile: tuple | None = None   # (tx, ty, tw, th), any origin
    half: bool = False          # also render RGBA16F output
    crop: tuple | None = None   # the tile the CPU reference checks (long rays: a few pixels of the frame)
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.den.shape[:3]
        return nx, ny, nz

    @property
    def divergent(self):
        return "divergent" in self.tags

    @property
    def edge(self):
        return "edge" in self.tags

    def __repr__(self):
        return (f"Case({self.name}: dims={self.dims} {self.W}x{self.H} tile={self.tile} dt={self.dt} camera kind {self.kind} "
                f"{'divergent ' if self.divergent else ''}tags={self.tags})")


def opacity_term_zero(a):
    """smoothstep(0, 0.7, a^3) == 0 in f32 (np_compute_reference.opacity)."""
    from np_compute_reference import opacity

    return opacity(np.asarray(a, np.float16).astype(np.float32)) == 0


def divergent(den, nrm):
    """The records whose short-form shade differs from the text's and can reach the colour (see the module's docstring)."""
    n = nrm.astype(np.float32)
    with np.errstate(invalid="ignore"):
        odd = (~np.isfinite(n[..., 0]) | ~np.isfinite(n[..., 2])) & (n[..., 1] < 0)
        return odd & (~opacity_term_zero(den[..., 3]) | (n[..., 1] == -np.inf))


def _calm(den, nrm):
    """Take the divergent records out of a volume meant for the records == literal twin check: their normal x and z become finite."""
    bad = divergent(den, nrm)
    nb = nrm.view(np.uint16)
    for k in (0, 2):
        nb[..., k][bad] = 0x3400  # 0.25
    return nrm


def _grid(dims):
    nx, ny, nz = dims
    return np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")


def _balls(rng, dims, count, rmax=0.35):
    z, y, x = _grid(dims)
    out = []
    for _ in range(count):
        c = rng.uniform(0.15, 0.85, 3) * np.array(dims)
        rad = rng.uniform(1.0, max(1.5, rmax * min(dims)))
        out.append((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 < rad * rad)
    return out


def _air(rng, dims, nan_normals=0.5):
    """Air: colour in [0, 1), opacity exactly +0 / -0 / -0.25 / another zero-term pattern, normals in [-1, 1) and NaN (all three
    components, the xor generator's holes) in a share `nan_normals`; the normals' w is drawn too (the records overwrite it)."""
    shape = dims[::-1]
    den = rng.random(shape + (4,), np.float32).astype(np.float16)
    op = rng.choice(np.array([0x0000, 0x8000, 0xB400] + list(ZERO_OPACITY_BITS), np.uint16), shape)
    den.view(np.uint16)[..., 3] = op
    nrm = (rng.random(shape + (4,), np.float32) * 2 - 1).astype(np.float16)
    nrm[rng.random(shape) < nan_normals, :3] = np.nan
    return den, nrm


def _blobs(rng, den, nrm, count, lo=0.2, rmax=0.35):
    dims = den.shape[:3][::-1]
    for ball in _balls(rng, dims, count, rmax):
        den[..., 3][ball] = np.float16(rng.uniform(lo, 1.0))
        nrm[ball, :3] = (rng.random((int(ball.sum()), 3)) * 2 - 1).astype(np.float16)
    return den, nrm


def _sprinkle(rng, a, bits, p):
    """Set a share p of the entries of the u16 view `a` to patterns drawn from `bits`, and each pattern at least once where it fits."""
    m = rng.random(a.shape) < p
    a[m] = rng.choice(np.array(bits, np.uint16), int(m.sum()))
    if a.size >= 4 * len(bits):
        a.flat[rng.choice(a.size, len(bits), replace=False)] = bits
    return a


def _p(dims):
    return 0.03 if np.prod(dims) > 64 else 0.3


def v_blobs(O, rng, dims):
    """The existing fuzz's volumes: blobs of opacity 0.2..1 in air of zero opacity with NaN normals in half of it."""
    return _blobs(rng, *_air(rng, dims), 3)


def v_edge_colour(O, rng, dims):
    """Edge patterns in each colour channel, on their own, in the air and in the blobs."""
    den, nrm = _blobs(rng, *_air(rng, dims), 2)
    for k in range(3):
        _sprinkle(rng, den.view(np.uint16)[..., k], EDGE_BITS, _p(dims) / 3)
    return den, nrm


def v_edge_opacity(O, rng, dims):
    """Opacity edge patterns and both sides of the zero point of smoothstep(0, 0.7, a^3)."""
    den, nrm = _blobs(rng, *_air(rng, dims), 2)
    _sprinkle(rng, den.view(np.uint16)[..., 3], EDGE_BITS + TINY_OPACITY_BITS + ZERO_OPACITY_BITS, 2 * _p(dims))
    return den, nrm


def v_edge_normals(O, rng, dims):
    """Edge patterns in each normal component on its own (never a divergent record: see _calm)."""
    den, nrm = _blobs(rng, *_air(rng, dims, 0.25), 2)
    for k in range(3):
        _sprinkle(rng, nrm.view(np.uint16)[..., k], EDGE_BITS, _p(dims) / 2)
    return den, _calm(den, nrm)


def v_nonfinite_air(O, rng, dims):
    """Air whose zero-weight step is NaN: a non-finite colour channel or a -inf normal component, and blobs."""
    den, nrm = _blobs(rng, *_air(rng, dims), 2)
    air = opacity_term_zero(den[..., 3])
    m = air & (rng.random(air.shape) < 0.02)
    k = rng.integers(0, 4, int(m.sum()))
    vals = rng.choice(np.array(NONFINITE_BITS, np.uint16), int(m.sum()))
    comp = rng.integers(0, 3, int(m.sum()))  # (the normal component of each -inf)
    idx = np.nonzero(m)
    for j in range(3):
        sel = k == j
        den.view(np.uint16)[idx[0][sel], idx[1][sel], idx[2][sel], j] = vals[sel]
    sel = k == 3
    nrm.view(np.uint16)[idx[0][sel], idx[1][sel], idx[2][sel], comp[sel]] = 0xFC00
    return den, _calm(den, nrm)


def v_xor(O, rng, dims):
    """The xor generator's volumes (NaN normals where the gradient vanishes) at a drawn time."""
    return O.volume_xor(dims, float(rng.choice([0.0, 0.37, 2.5, 1000.0])))


def v_all_edges(O, rng, dims):
    """Every half of every record drawn from the edge patterns (dense: rays end early or turn NaN)."""
    shape = dims[::-1] + (4,)
    bits = np.array(EDGE_BITS + TINY_OPACITY_BITS, np.uint16)
    den = rng.choice(bits, shape).view(np.float16)
    nrm = rng.choice(bits, shape).view(np.float16)
    return den, _calm(den, nrm)


VOLUMES = {"blobs": v_blobs, "edge colour": v_edge_colour, "edge opacity": v_edge_opacity, "edge normals": v_edge_normals,
           "non-finite air": v_nonfinite_air, "xor": v_xor, "all edges": v_all_edges}
EDGE_KINDS = ("edge colour", "edge opacity", "edge normals", "non-finite air", "all edges")


def _far_image(zoom):
    """Image and tile for an eye `zoom` units from the box: the box covers about W / zoom pixels each way (the compute twin's rays:
    90-degree fovy, y scaled by H / W); W = 22 zoom puts ~22 x 22 pixels on it, the tile holds them."""
    W = int(22 * zoom)
    c = 15
    H = 2 * c + 6
    return W, H, (W // 2 - c, H // 2 - c, 2 * c, 2 * c)


def _camera(rng, kind, W, H):
    """The four kinds of tests/table_cases.py centred on the compute twin's [-1, 1] box, and far eyes."""
    if kind == 0:    # ordinary orbit
        return (float(rng.uniform(1.8, 4.5)), float(rng.uniform(-1.4, 1.4)), float(rng.uniform(0, 6.28)), (0.0, 0.0, 0.0), W / H)
    if kind == 1:    # eye inside the box
        return (float(rng.uniform(0.1, 0.7)), float(rng.uniform(-1.0, 1.0)), float(rng.uniform(0, 6.28)),
                tuple(float(v) for v in rng.uniform(-0.4, 0.4, 3)), W / H)
    if kind == 2:    # axis-aligned: direction components that are exactly zero on the centre rays
        return (3.0, 0.0, float(rng.integers(0, 4)) * 1.5707963, (0.0, 0.0, 0.0), 1.0)
    if kind == 3:    # grazing a face
        return (2.4, float(rng.uniform(-0.05, 0.05)), float(rng.uniform(0, 6.28)), (0.0, float(rng.choice([-0.96, 0.96])), 0.0), W / H)
    return (float(rng.uniform(10.0, 60.0)), float(rng.uniform(-1.2, 1.2)), float(rng.uniform(0, 6.28)),
            tuple(float(v) for v in rng.uniform(-0.2, 0.2, 3)), 1.0)


def _random_dims(rng, hi):
    near = [v for v in range(1, hi + 1) if (v % 4) in (1, 3)]
    return tuple(int(rng.choice(near)) if rng.random() < 0.6 else int(rng.integers(1, hi + 1)) for _ in range(3))


def _walk_volume(rng, dims, nblobs):
    """A large volume of air (zero opacity; NaN normals in half of it) with `nblobs` small blobs."""
    den, nrm = _air(rng, dims)
    z, y, x = _grid(dims)
    for _ in range(nblobs):
        c = rng.uniform(0.1, 0.9, 3) * np.array(dims)
        r = rng.uniform(1.5, 4.0)
        ball = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 < r * r
        den[..., 3][ball] = np.float16(rng.uniform(0.3, 0.9))
        nrm[ball, :3] = (rng.random((int(ball.sum()), 3)) * 2 - 1).astype(np.float16)
    return den, nrm


# the camera's view direction is (sin(yaw) cos(pitch), sin(pitch), cos(yaw) cos(pitch)) (oracle: vo_camera_eye): (pitch, yaw) looking down +x,
# +y (a little off the pole, where look_at's up vector would be degenerate) and +z
AXIS_VIEW = {0: (0.0, 1.5707963), 1: (1.45, 0.0), 2: (0.0, 0.0)}


def _along(axis, far, rng):
    """A camera looking down `axis` (0 x, 1 y, 2 z) from `far` units, a little off the axis."""
    pitch, yaw = AXIS_VIEW[axis]
    return (far, pitch + float(rng.uniform(-0.05, 0.05)), yaw + float(rng.uniform(-0.05, 0.05)), (0.0, 0.0, 0.0), 1.0)


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    cases = []
    vkinds = tuple(VOLUMES)

    def add(name, den, nrm, cam, kind, W, H, dt, tags=(), **kw):
        tags = tuple(tags) + (("divergent",) if divergent(den, nrm).any() else ())
        cases.append(Case(name, den, nrm, cam, kind, W, H, dt, tags=tags, **kw))

    for trial in range(N_RANDOM):
        dt = DTS[trial % len(DTS)]
        vkind = vkinds[trial % len(vkinds)]
        kind = trial % 5
        dims = _random_dims(rng, 16 if dt < 0.1 else 72)  # (the smallest step: ~3000 iterations per ray over 16 voxels)
        tile = None
        if kind == 4:
            cam = _camera(rng, 4, 1, 1)
            W, H, tile = _far_image(cam[0])
            if dt < 0.1 and cam[0] > 50:  # (the library refuses a dt that cannot advance t at this distance: dt_scale >= 0.025)
                dt = 0.03
        else:
            W, H = int(rng.integers(24, 73)), int(rng.integers(24, 73))
            if dt < 0.1:
                W, H = min(W, 36), min(H, 36)
            cam = _camera(rng, kind, W, H)
        den, nrm = VOLUMES[vkind](O, rng, dims)
        tags = (vkind, "random dims") + (("edge",) if vkind in EDGE_KINDS else ())
        add(f"r{trial:02d}", den, nrm, cam, kind, W, H, dt, tags, tile=tile, half=trial % 6 == 4)
    # dims that straddle the 4^3 record bricks; volumes of one voxel and of one voxel per axis
    for j, dims in enumerate(FIXED_DIMS):
        vkind = vkinds[(3 * j + 1) % len(vkinds)]
        W, H = (40, 32) if j % 2 else (33, 41)
        add(f"dims{'x'.join(map(str, dims))}", *VOLUMES[vkind](O, rng, dims), _camera(rng, j % 4, W, H), j % 4, W, H,
            DTS[(j + 2) % len(DTS)], (vkind, "fixed dims") + (("edge",) if vkind in EDGE_KINDS else ()))
    # the zero-weight steps that are NaN, one kind at a time in air around a blob: the records' skip map must not walk over them
    for name, half, k, bits in (("NaN colour in the air", 0, 1, 0x7E01), ("+inf colour in the air", 0, 0, 0x7C00),
                                ("-inf colour in the air", 0, 2, 0xFC00), ("-inf normal y in the air", 1, 1, 0xFC00),
                                ("-inf normal x in the air", 1, 0, 0xFC00)):
        dims = (36, 28, 32)
        den, nrm = _air(rng, dims, 0.0)
        _blobs(rng, den, nrm, 1, rmax=0.2)
        air = opacity_term_zero(den[..., 3])
        m = air & (rng.random(air.shape) < 0.01)
        (den if half == 0 else nrm).view(np.uint16)[..., k][m] = bits
        if half == 1:
            nrm.view(np.uint16)[..., 1][m & (nrm[..., 1] < 0)] = 0x3400 if k != 1 else 0xFC00  # (keep them out of `divergent`)
        add(name, den, nrm, _camera(rng, 0, 48, 40), 0, 48, 40, 1.0, ("edge", "non-finite air"), half=k == 1)
    # the xor generator's volumes at the example's camera and at the box's edges
    den, nrm = O.volume_xor(64, 0.0)
    add("xor 64", den, nrm, (3.0, -0.5, 1.0, (0.0, 0.0, 0.0), 64 / 40), 0, 64, 40, 1.0, ("xor",), half=True)
    add("xor 37x50x29 inside", *O.volume_xor((37, 50, 29), 0.5), _camera(rng, 1, 40, 40), 1, 40, 40, 0.5, ("xor",))
    # walks: small blobs in 128..256 voxels of air along the ray, hops of up to the 61-voxel skip radius; the 0.01 dt floor binds
    for name, dims, axis, far, dt, nb in (("walk x 160", (160, 20, 24), 0, 3.0, 1.0, 4), ("walk y 200", (18, 200, 22), 1, 2.5, 0.5, 5),
                                          ("walk z 256", (16, 14, 256), 2, 3.5, 0.15, 3), ("walk x 128 far", (128, 16, 16), 0, 40.0, 0.3, 3)):
        den, nrm = _walk_volume(rng, dims, nb)
        W, H, tile = _far_image(far) if far > 10 else (48, 40, None)
        add(name, den, nrm, _along(axis, far, rng), 4 if far > 10 else 0, W, H, dt, ("walk",), tile=tile,
            crop=(W // 2 - 2, H // 2 - 2, 4, 4) if far > 10 else (20, 16, 8, 8))
    # far eyes down the 256-voxel x axis at the smallest steps the library allows there (the 0.01 floor binds: dt = 0.01 dt_scale): each
    # t = t + dt rounds up by ~0.48 ulp (dt / ulp(t) = k + 0.52; DRIFT_ULPS), so t runs ~1.4 % (t ~ 45) and ~3 % (t ~ 150) ahead of i * dt
    for name, far, dts in (("far t~45 drift", 45.0, DRIFT_ULPS["far t~45 drift"] / 2621.44),
                           ("far t~150 drift", 150.0, DRIFT_ULPS["far t~150 drift"] / 655.36)):
        den, nrm = _walk_volume(rng, (256, 12, 12), 6)
        W, H, tile = _far_image(far) if far < 100 else (1200, 24, (588, 0, 24, 24))
        add(name, den, nrm, _along(0, far, rng), 4, W, H, dts, ("walk", "far"), tile=tile, crop=(W // 2 - 1, H // 2 - 1, 2, 2))
    # the same drift against one slab: air down 256 voxels of x (no record that can contribute, so the skip map saturates at 61) and a
    # 4-voxel slab of opacity 0.5 across the whole section at x = K.  The second hop's plan ends two voxels short of the slab; a sample that
    # runs 1.7 (eye 150: each step 1.03 dt) or 3.5 voxels (eye 300: 1.06 dt) ahead of it lands in the slab unless the hop is shortened
    for name, far, dts, K in (("slab at 115, eye 150", 150.0, DRIFT_ULPS["slab at 115, eye 150"] / 655.36, 115),
                              ("slab at 110, eye 300", 300.0, DRIFT_ULPS["slab at 110, eye 300"] / 327.68, 110)):
        den, nrm = _air(rng, (256, 12, 12))
        den[:, :, K:K + 4, 3] = np.float16(0.5)
        nrm[:, :, K:K + 4, :3] = np.float16(0.25)
        W = int(10 * far)
        cam = (far, 0.01, 1.5707963 + 0.013, (0.0, 0.0, 0.0), 1.0)
        add(name, den, nrm, cam, 4, W, 16, dts, ("walk", "far", "slab"), tile=(W // 2 - 4, 4, 8, 8), crop=(W // 2 - 1, 7, 2, 2))
    # records that hold a divergent normal: the records-vs-records equalities and the literal twin against the oracle only
    den, nrm = _blobs(rng, *_air(rng, (30, 26, 34)), 3)
    b = _balls(rng, (30, 26, 34), 1)[0]
    nrm.view(np.uint16)[..., 0][b] = rng.choice(np.array([0x7C00, 0xFC00, 0x7E00], np.uint16), int(b.sum()))
    nrm[..., 1][b] = -np.abs(nrm[..., 1][b])
    den[..., 3][b] = np.float16(0.6)
    add("inf normal x, y < 0", den, nrm, _camera(rng, 0, 44, 36), 0, 44, 36, 0.5, ("edge",))
    # tiles: one that starts off screen, one inside, one past the far corner, one wholly off screen
    cam = (2.6, 0.4, 0.8, (0.0, 0.0, 0.0), 64 / 48)
    add("tile at a negative origin", *v_edge_colour(O, rng, (37, 29, 41)), cam, 0, 64, 48, 0.5, ("edge",), tile=(-9, -6, 40, 30))
    add("tile inside", *v_nonfinite_air(O, rng, (29, 35, 30)), cam, 0, 64, 48, 1.0, ("edge",), tile=(13, 7, 31, 22), half=True)
    add("tile past the corner", *v_blobs(O, rng, (30, 30, 30)), cam, 0, 64, 48, 1.7, tile=(40, 30, 40, 40))
    add("tile off screen", *v_blobs(O, rng, (20, 20, 20)), cam, 0, 64, 48, 1.0, tile=(64, 0, 32, 32))
    return tuple(cases)


N_CASES = N_RANDOM + len(FIXED_DIMS) + 5 + 2 + 4 + 2 + 2 + 1 + 4


def cases(O):
    """The case list (deterministic: built once from SEED).  O: the oracle module (tests' `O` fixture)."""
    out = _cases(O)
    assert len(out) == N_CASES, len(out)
    return out


# ---- C3: the procedural mode (no volume): cameras, dt and tiles drawn as above, Uniform.time up to 1e5

PROC_TIMES = (0.0, 0.75, 3.0, 100.0, 4096.5, 1.0e5)


@functools.lru_cache(maxsize=None)
def procedural_cases():
    """(name, cam, kind, W, H, dt, tile, time, half) for ~10 C3 renders."""
    rng = np.random.default_rng(SEED + 3)
    out = []
    for j in range(10):
        kind = j % 5
        dt = DTS[(j + 1) % len(DTS)]
        tile = None
        if kind == 4:
            cam = _camera(rng, 4, 1, 1)
            W, H, tile = _far_image(cam[0])
            dt = max(dt, 0.3)
        else:
            W, H = int(rng.integers(24, 57)), int(rng.integers(24, 57))
            cam = _camera(rng, kind, W, H)
            if j % 3 == 2:
                tile = (int(rng.integers(-16, W)), int(rng.integers(-16, H)), 32, 24)
        if dt < 0.1:
            W, H = min(W, 24), min(H, 24)
        out.append((f"c3 {j}", cam, kind, W, H, dt, tile, PROC_TIMES[j % len(PROC_TIMES)], j % 3 == 1))
    return tuple(out)
