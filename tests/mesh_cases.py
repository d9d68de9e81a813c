"""The shared case list of the mesh tests (vk_extract_isosurface): small volumes of the three formats -- the dimensions
are the histogram's, with 2x2x2 added as the smallest volume that has a cube -- and for each a set of voxel boxes.  The CPU suite holds the C
restatement to the numpy reference over it (tests/test_mesh_fuzz_cpu.py), the GPU suite every layout's kernels to the restatement
(tests/test_mesh_fuzz_gpu.py).  A volume is shared by its boxes (`vol_id`): the GPU driver uploads it once per layout.

iso is in sample values.  0.5 gives iso_k = 127.5 on R8 and 32767.5 on R16_UNORM, both exact: a half-integer on integer data, so no vertex
lands on a lattice point.  1.0 gives 255 and 65535, 0.25 is itself: thresholds that stored values hit exactly (f == 0 and f == 1)."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name vol_id kind vol box iso")

DIMS = ((1, 1, 1), (2, 2, 2), (5, 3, 2), (17, 9, 6), (24, 24, 24), (33, 20, 7))  # nx, ny, nz
DTYPE = {"u8": np.uint8, "u16": np.uint16, "f16": np.float16}
TOP = {"u8": 255, "u16": 65535, "f16": 1.0}


def boxes(nx, ny, nz):
    """(name, box): the whole volume (None), an empty box, a box one voxel thick (no cubes), an odd origin, the low and the high faces."""
    out = [("whole", None), ("empty", ((nx // 2, 0, 0), (nx // 2, ny, nz))), ("one voxel thick", ((0, 0, nz // 2), (nx, ny, nz // 2 + 1)))]
    if min(nx, ny, nz) >= 2:
        out.append(("odd origin", ((1, 1, 1), (nx, ny, nz))))
        out.append(("low faces", ((0, 0, 0), (nx // 2 + 1, ny // 2 + 1, nz // 2 + 1))))
        out.append(("high faces", ((nx // 2, ny // 2, nz // 2), (nx, ny, nz))))
    return out


def _grid(d):
    """Voxel centres of a volume of dims d = (nx, ny, nz) in [-1, 1]^3, as arrays [nz, ny, nx]."""
    ax = [(np.arange(n) + 0.5) / n * 2.0 - 1.0 for n in d]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return x, y, z


def quantise(g, kind):
    """A field in [0, 1] as stored texels."""
    if kind == "f16":
        return g.astype(np.float16)
    return np.rint(g * TOP[kind]).astype(DTYPE[kind])


def ball(d, kind):
    """1.3 - 1.6 r clipped to [0, 1], r the distance from the centre in half-extents: 0 on the volume's faces, 0.5 at r = 0.5."""
    x, y, z = _grid(d)
    return quantise(np.clip(1.3 - 1.6 * np.sqrt(x * x + y * y + z * z), 0.0, 1.0), kind)


def torus(d, kind):
    """1 - dist / 0.4 clipped, dist the distance from the ring of radius 0.55 in the z = 0 plane: 0.5 at dist = 0.2, 0 on the faces."""
    x, y, z = _grid(d)
    dist = np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)
    return quantise(np.clip(1.0 - dist / 0.4, 0.0, 1.0), kind)


def volumes():
    """(vol_id, kind, vol [nz, ny, nx], iso)."""
    rng = np.random.default_rng(21)
    out = []

    def shape(d):
        return (d[2], d[1], d[0])

    for kind in ("u8", "u16", "f16"):
        dt, top = DTYPE[kind], TOP[kind]
        at = 0.25 if kind == "f16" else 1.0  # a threshold the two-valued volume hits exactly
        out.append((f"{kind} 1x1x1 constant", kind, np.full(shape(DIMS[0]), top, dt), 0.5))
        out.append((f"{kind} 17x9x6 constant", kind, np.full(shape(DIMS[3]), top, dt), 0.5))
        out.append((f"{kind} 2x2x2 two-valued", kind, np.array([0, top, top, 0, top, 0, 0, 0], dt).reshape(2, 2, 2), 0.5))
        hi = np.float16(0.25) if kind == "f16" else top
        out.append((f"{kind} 33x20x7 two-valued at iso_k", kind, rng.choice(np.array([0, hi], dt), shape(DIMS[5]), p=(0.7, 0.3)), at))
        if kind == "f16":
            out.append((f"{kind} 5x3x2 uniform", kind, rng.uniform(0.0, 1.0, shape(DIMS[2])).astype(dt), 0.5))
            out.append((f"{kind} 24^3 uniform", kind, rng.uniform(-1.0, 2.0, shape(DIMS[4])).astype(dt), 0.5))
        else:
            out.append((f"{kind} 5x3x2 uniform", kind, rng.integers(0, top + 1, shape(DIMS[2])).astype(dt), 0.5))
            out.append((f"{kind} 24^3 uniform", kind, rng.integers(0, top + 1, shape(DIMS[4])).astype(dt), 0.5))
        out.append((f"{kind} 17x9x6 ball", kind, ball(DIMS[3], kind), 0.5))
        out.append((f"{kind} 24^3 ball", kind, ball(DIMS[4], kind), 0.5))
    out.append(("u8 24^3 torus", "u8", torus(DIMS[4], "u8"), 0.5))
    out.append(("u16 33x20x7 torus", "u16", torus(DIMS[5], "u16"), 0.5))
    # u8 values of a narrow range around a threshold that is an integer: many corners exactly at iso_k = 51 (0.2f * 255f rounds to 51)
    out.append(("u8 33x20x7 narrow band around iso_k", "u8", rng.integers(49, 54, shape(DIMS[5])).astype(np.uint8), 0.2))
    v = rng.uniform(-1.0, 1.5, shape(DIMS[3])).astype(np.float16)
    flat = v.ravel()
    special = [np.float16(np.nan), np.float16(np.inf), np.float16(-np.inf), np.float16(-0.0), np.float16(0.0), np.float16(6e-8), np.float16(-6e-8), np.float16(3e-5),
               np.float16(0.25), np.float16(65504.0), np.float16(-65504.0)]
    for rep in range(3):
        for k, s in enumerate(special):
            flat[(rep * 307 + k * 29 + 3) % flat.size] = s
    out.append(("f16 17x9x6 NaN, inf, -0, subnormals", "f16", v, 0.25))
    w = rng.uniform(-1e-4, 1e-4, shape(DIMS[5])).astype(np.float16)  # subnormals and -0 around a threshold of 0
    w.ravel()[::7] = np.float16(-0.0)
    w.ravel()[3::11] = np.float16(0.0)
    w.ravel()[5::501] = np.float16(np.nan)
    out.append(("f16 33x20x7 subnormals and signed zeros around iso 0", "f16", w, 0.0))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        out = []
        for vol_id, kind, vol, iso in volumes():
            nz, ny, nx = vol.shape
            for bname, box in boxes(nx, ny, nz):
                out.append(Case(f"{vol_id}, {bname}, iso {iso}", vol_id, kind, vol, box, iso))
        _CASES = out
    return _CASES
