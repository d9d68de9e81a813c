"""The cases of the geometry pass of the first-hit isosurface (vk_render_geometry), shared by
tests/test_geom_fuzz_cpu.py (the numpy reference against the C restatement) and tests/test_geom_fuzz_gpu.py (the kernels against the C
restatement).

The pass is the isosurface colour render's ray, so its cases are that render's: every case of tests/iso_cases.py (u8 and f16, with the
lights they carry: lighting both off and on, which the pass must ignore), the isosurface cases of tests/u16_cases.py (R16_UNORM, some
under a clip box) and of tests/clip_cases.py (the boxes and cameras of the clip-box tests).  Named cases pin the pass's own edges: a
1x1x1 volume, a tile at a negative origin under a box, first-iteration hits on a clip face, R = 0 and R = 16, a threshold above all data
(every record a miss), a hit on a +inf tap, and NaN samples passed over on the way to a hit.  Frames are 24-80 px, dims the existing small ones."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import clip_cases as CC
import iso_cases
import u16_cases as UC
from shadow_cases import two_balls

LIGHT = dict(direction=(0.3, 1.0, 0.5), ambient=0.2, diffuse=0.8, specular=0.4, shininess=16.0)


@dataclass
class Case:
    name: str
    vol: np.ndarray            # (nz, ny, nx) u8, f16 or uint16 (R16_UNORM)
    cam: tuple                 # arguments of oracle.camera_blob
    W: int
    H: int
    dt: float
    iso: float                 # threshold in sample values
    refine: int = 4
    light: dict | None = None  # keyword arguments of Context.set_lighting: set on the context, and without influence
    box: tuple | None = None   # (lo3, hi3)
    tile: tuple | None = None
    tags: tuple = field(default_factory=tuple)

    @property
    def dims(self):
        nz, ny, nx = self.vol.shape
        return nx, ny, nz

    @property
    def kind(self):
        return {np.dtype(np.uint8): "u8", np.dtype(np.float16): "f16", np.dtype(np.uint16): "u16"}[self.vol.dtype]

    def __repr__(self):
        return (f"GeomCase({self.name}: dims={self.dims} {self.kind} {self.W}x{self.H} tile={self.tile} dt={self.dt} iso={self.iso} R={self.refine} "
                f"lit={self.light is not None} box={self.box})")


def _f16_slabs(front, back):
    """A (nz, ny, nx) = (20, 18, 24) f16 volume, 0 but for a slab of `front` at x = 8..9 and one of `back` from x = 14 on: seen along +x
    from the low-x side a ray passes the first slab before it reaches the second."""
    v = np.zeros((20, 18, 24), np.float16)
    v[:, :, 8:10] = front
    v[:, :, 14:] = back
    return v


@functools.lru_cache(maxsize=None)
def _cases(O):
    out = []
    for c in iso_cases.cases(O):
        out.append(Case("iso " + c.name, c.vol, c.cam, c.W, c.H, c.dt, c.iso, c.refine, c.light, None, c.tile, ("iso",) + tuple(c.tags)))
    for c in UC.cases(O):
        if c.family == "iso":
            out.append(Case("u16 " + c.name, c.vol, c.cam, c.W, c.H, c.dt, c.iso, c.refine, c.light, c.box, None, ("u16",) + tuple(c.tags)))
    for c in CC.CASES:
        if c.family in ("iso", "iso lit"):
            out.append(Case("clip " + c.name, CC.volumes(O)[c.volume], CC.CAMERAS[c.camera], CC.W, CC.H, c.dt, CC.ISO[c.volume], 4,
                            CC.LIGHT_X if c.family == "iso lit" else None, CC.BOXES[c.box], c.tile, ("clip",)))
    side = (0.7, 0.2, 0.0, (0.5, 0.5, 0.5), 64 / 48)
    corner = (1.6, 0.6, 0.8, (0.5, 0.5, 0.5), 48 / 40)
    # one voxel: every tap is the same, every hit is a first-iteration hit without a gradient
    out.append(Case("1x1x1", np.full((1, 1, 1), 200, np.uint8), corner, 40, 32, 0.5, 0.5, 4, None))
    # a tile that starts off screen, under a box, lit
    out.append(Case("tile at a negative origin, clip box", two_balls((37, 29, 41)), side, 64, 48, 0.5, 0.4, 4, LIGHT, ((0.1, 0.0, 0.2), (0.9, 1.0, 0.8)),
                    (-9, -6, 48, 40)))
    # the threshold below all data under a box: every ray through the box hits in its first iteration, on the cut face of the clip box
    out.append(Case("first-iteration hits on a clip face", O.volume_standin_u8((40, 33, 27), seed=11), corner, 48, 40, 0.5, -0.5, 16, None,
                    ((0.2, 0.1, 0.15), (0.8, 0.9, 0.7))))
    # no bisection, and the deepest one, over coarse steps: the crossing lies anywhere within the step
    out.append(Case("R = 0", two_balls((36, 30, 34)), side, 48, 40, 1.7, 0.5, 0, LIGHT))
    out.append(Case("R = 16", two_balls((36, 30, 34)), side, 48, 40, 1.7, 0.5, 16, None))
    # the threshold above all data: every record is the miss record
    out.append(Case("iso above all data", O.volume_standin_u8((33, 17, 65), seed=9), corner, 48, 40, 0.5, 2.0, 4, LIGHT))
    # a lattice of +inf voxels in zeros: the filter gives +inf only in the cell that holds such a voxel at its high corner on every axis
    # (fma(f, inf - 0, 0) per lerp; with the voxel at any other corner a lerp meets inf - inf or f * -inf: NaN, no hit), +inf >= iso_k hits
    lattice = np.zeros((20, 18, 24), np.float16)
    lattice[2::3, 2::3, 2::3] = np.inf
    out.append(Case("+inf tap hit", lattice, (1.4, 0.1, 1.5707963, (0.5, 0.5, 0.5), 40 / 32), 40, 32, 0.5, 0.5, 4, None))
    # a slab of NaN in front of a solid: the samples in it are NaN, no hit, and the ray goes on to the solid behind
    out.append(Case("NaN samples passed over", _f16_slabs(np.nan, 1.0), (1.4, 0.1, 1.5707963, (0.5, 0.5, 0.5), 40 / 32), 40, 32, 0.5, 0.5, 4, LIGHT))
    return tuple(out)


N_NAMED = 8


def cases(O):
    """The case list (deterministic).  O: the oracle module (tests' `O` fixture)."""
    out = _cases(O)
    n_u16 = sum(c.family == "iso" for c in UC.cases(O))
    n_clip = sum(c.family in ("iso", "iso lit") for c in CC.CASES)
    assert len(out) == iso_cases.N_CASES + n_u16 + n_clip + N_NAMED, len(out)
    return out
