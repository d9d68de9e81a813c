"""The boxes, cameras, volumes and families of the clip-box tests (vk_set_clip_box), shared by tests/test_clip_cpu.py (the references under a
box, on the CPU) and tests/test_clip_gpu.py (the kernels against them).

Boxes: the unit cube, a half-space, a region of interest off the voxel grid, a box on 4-voxel brick boundaries of the 32^3 volume, a slab
thinner than a voxel and a slab thinner than one step.  Cameras: an orbit, an axis-aligned view, the eye inside the box, the eye inside the
cube but outside the box, and a view grazing a box face (and, as a deliberate miss, the eye looking away from the box).  Volumes: the 32^3 u8 stand-in, an f16 fog of (33, 17, 65) and a (5, 4, 9) u8
volume.  Families: table, lit, MAX with and without a table, isosurface lit and unlit."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import np_clip_reference as NC

W, H = 48, 40
UNIT = NC.UNIT
HALF = ((0.5, 0.0, 0.0), (1.0, 1.0, 1.0))
ROI = ((0.25, 0.3, 0.1), (0.8, 0.75, 0.6))
BRICKS = ((0.125, 0.25, 0.375), (0.75, 0.625, 1.0))   # multiples of 4 / 32: 4-voxel brick boundaries of the 32^3 volume
THIN_VOXEL = ((0.0, 0.0, 0.49), (1.0, 1.0, 0.51))     # 0.02 < 1 / 32
THIN_STEP = ((0.0, 0.5, 0.0), (1.0, 0.505, 1.0))      # 0.005: thinner than one step at every dt used (dt 0.15 / 32 = 0.0047 along an axis)
BOXES = {"unit": UNIT, "half-space": HALF, "roi": ROI, "bricks": BRICKS, "thin voxel": THIN_VOXEL, "thin step": THIN_STEP}

# arguments of oracle.camera_blob: zoom (the eye's distance from the target), pitch, yaw, target, aspect
CAMERAS = {
    "orbit": (1.3, 0.45, 0.9, (0.5, 0.5, 0.5), W / H),
    "axis": (1.5, 0.0, 1.5707963, (0.5, 0.5, 0.5), 1.0),           # along +x: direction components that are exactly zero on the centre rays
    "axis z": (1.5, 0.0, 0.0, (0.5, 0.5, 0.5), 1.0),               # along +z: the z slab face-on
    "eye in box": (0.12, 0.3, 4.5, (0.6, 0.5, 0.35), W / H),       # the eye inside ROI, HALF and the unit cube, looking towards -x: HALF's cut face 0.2 ahead
    "eye in cube": (0.64, -0.675, 1.65, (0.6, 0.5, 0.5), W / H),   # the eye at (0.10, 0.90, 0.54): inside the cube, outside every box above, looking into them
    "eye in cube, away": (0.1, -0.2, 4.0, (0.12, 0.85, 0.8), W / H),  # ... and looking away from them
    "grazing": (1.2, 0.02, 0.0, (0.5, 0.75, 0.35), W / H),         # the eye 0.024 above the plane y = 0.75, ROI's upper face, looking along z
}

LIGHT = dict(direction="headlight", ambient=0.3, diffuse=0.7, specular=0.2, shininess=24.0)
LIGHT_X = dict(direction=(1.0, 0.4, -0.3), ambient=0.2, diffuse=0.8, specular=0.4, shininess=8.0)


def table(n=16, seed=7):
    """A faint table, clear at the low end (the air: cells to skip), so that rays run long and a cut shows the inside."""
    rng = np.random.default_rng(seed)
    t = np.empty((n, 4), np.float32)
    t[:, :3] = rng.uniform(0.05, 1.0, (n, 3))
    t[:, 3] = np.linspace(0.0, 0.35, n) ** 2
    t[: n // 4, 3] = 0.0
    return t


@dataclass
class Case:
    name: str
    family: str                # "table" | "lit" | "mip" | "mip table" | "iso" | "iso lit"
    volume: str                # key of volumes()
    box: str
    camera: str
    dt: float
    tile: tuple | None = None
    miss: bool = False         # a deliberate miss: the picture may be empty
    half: bool = False         # also rendered to RGBA16F
    tags: tuple = field(default_factory=tuple)

    def __repr__(self):
        return f"ClipCase({self.name}: {self.family} / {self.volume} / box {self.box} / {self.camera} / dt {self.dt} / tile {self.tile})"


@functools.lru_cache(maxsize=None)
def volumes(O):
    """name -> (nz, ny, nx) array; read-only."""
    rng = np.random.default_rng(20261019)
    fog = (0.15 + 0.5 * rng.random((65, 17, 33)) * (np.linspace(0.0, 1.0, 33)[None, None, :] ** 0.5)).astype(np.float16)  # finite, thicker towards +x
    small = rng.integers(0, 256, (9, 4, 5)).astype(np.uint8)
    out = {"standin32": O.volume_standin_u8(32), "fog f16": fog, "small": small}
    for v in out.values():
        v.setflags(write=False)
    return out


ISO = {"standin32": 0.3, "fog f16": 0.45, "small": 0.5}
DOMAIN = {"standin32": (0.0, 1.0), "fog f16": (0.1, 0.7), "small": (0.0, 1.0)}
FAMILIES = ("table", "lit", "mip", "mip table", "iso", "iso lit")


_REFERENCES = {}


def reference(O, c, box="case"):
    """(rgb float64 [H, W, 3], steps u32 [H, W]) of the case under its box (box=None: unclipped), from the numpy references.  Computed once
    per case and box and shared by the tests of a session: read-only."""
    key = (c.name, box if box is None or isinstance(box, str) else tuple(map(tuple, box)))
    if key not in _REFERENCES:
        _REFERENCES[key] = _reference(O, c, box)
        for a in _REFERENCES[key]:
            a.setflags(write=False)
    return _REFERENCES[key]


def tile_mask(c):
    m = np.ones((H, W), bool)
    if c.tile is not None:
        x, y, w, h = c.tile
        m[:] = False
        m[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = True
    return m


def _reference(O, c, box):
    vol = volumes(O)[c.volume]
    cam = O.camera_blob(*CAMERAS[c.camera])
    b = BOXES[c.box] if box == "case" else box
    kw = dict(dt=c.dt, tile=c.tile)
    if c.family in ("table", "lit"):
        return NC.render_table(b, cam, vol, W, H, table=table(), domain=DOMAIN[c.volume], light=LIGHT if c.family == "lit" else None, **kw)[:2]
    if c.family in ("mip", "mip table"):
        return NC.render_mip(b, cam, vol, W, H, table=table() if c.family == "mip table" else None, domain=DOMAIN[c.volume], **kw)[:2]
    return NC.render_iso(b, cam, vol, W, H, iso=ISO[c.volume], colour=(0.9, 0.7, 0.4), refine=4, light=LIGHT_X if c.family == "iso lit" else None, **kw)[:2]


def _cases():
    out = []
    fam = 0

    def add(name, volume, box, camera, dt, **kw):
        nonlocal fam
        family = kw.pop("family", None) or FAMILIES[fam % len(FAMILIES)]
        fam += 1
        out.append(Case(name, family, volume, box, camera, dt, **kw))

    # every box under the orbit and one other camera on the 32^3 stand-in, the families and step sizes dealt in turn
    dts = (0.5, 0.15, 1.7)
    for i, (box, cam2) in enumerate((("unit", "axis"), ("half-space", "eye in box"), ("roi", "grazing"), ("bricks", "eye in cube"), ("thin voxel", "axis z"),
                                     ("thin step", "eye in cube"))):
        add(f"{box} / orbit", "standin32", box, "orbit", dts[i % 3])
        add(f"{box} / {cam2}", "standin32", box, cam2, dts[(i + 1) % 3])
    # every family under the region of interest and the half-space
    for i, family in enumerate(FAMILIES):
        add(f"roi / {family}", "standin32", "roi", ("orbit", "eye in box", "axis")[i % 3], dts[i % 3], family=family, half=i % 2 == 0)
        add(f"half-space / {family}", "standin32", "half-space", ("axis", "orbit", "eye in cube")[i % 3], dts[(i + 2) % 3], family=family)
    # the eye inside the cube but outside the box, looking away from it: nothing to see
    add("roi behind the eye", "standin32", "roi", "eye in cube, away", 0.5, family="table", miss=True)
    # the f16 fog and the small volume: boxes off their grids
    for i, family in enumerate(FAMILIES):
        add(f"fog / {family}", "fog f16", ("roi", "half-space", "thin voxel")[i % 3], ("orbit", "eye in box", "axis z")[i % 3], dts[i % 3], family=family, half=i == 1)
    for i, family in enumerate(("table", "mip", "iso lit", "lit")):
        add(f"small / {family}", "small", ("roi", "half-space", "bricks", "thin step")[i], ("orbit", "axis", "orbit", "orbit")[i], dts[i % 3], family=family)
    # a tile that starts off screen
    add("tile off screen / table", "standin32", "roi", "orbit", 0.5, family="lit", tile=(-9, -6, 40, 30))
    add("tile off screen / iso", "standin32", "half-space", "orbit", 0.5, family="iso lit", tile=(-9, -6, 40, 30))
    return tuple(out)


CASES = _cases()
