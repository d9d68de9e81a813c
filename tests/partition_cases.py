"""The seeded fuzz cases of the code around the march -- the deal of a frame's tiles over ranks, the batched launch, the compact records on
the wire, the root's un-tile and its "over" form -- shared by tests/test_partition_fuzz_cpu.py (the numpy reference against the library's
host functions and against itself, and the conditions this list is built for) and tests/test_partition_fuzz_gpu.py (the kernels against
vk_render's frames, bit for bit), so that both walk the same list.

A case fixes the mode and volume, the frame size, the output format, the tile size, the wire format, the cameras of one or more consecutive
batches and a list of (nranks, root_skip) pairs.  Everything is small: the march is not the subject.  Output format and wire format are
dealt in cycles of lengths 2 and 3, frame sizes in a cycle of 11 (8 of them with an odd width, 6 with an odd height), tile sizes in a cycle
of 7, modes in a cycle of 5; the draw only fills in camera parameters.  The named cases pin what a draw may miss: a tile of 1024 pixels, batches
that mix a frame whose camera misses the box with a fully active one, batches in which every frame misses, more ranks than active tiles, and the
sequences of batches along which the over un-tile meets every transition of a tile (inactive / active in the batch named as `prev` and now)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from table_cases import _camera

SEED = 20261018
N_RANDOM = 30
WIRE_RGBA, WIRE_RGB = 0, 1
SIZES = ((97, 61), (33, 130), (129, 65), (7, 5), (1, 1), (8, 8), (64, 64), (120, 72), (97, 61), (33, 130), (7, 5))
TILES = (8, 16, 24, 40, 64, 128, 16)
MODES = ("naive u8", "naive f16", "compute", "procedural", "naive u8")
BATCHES = (1, 3, 4, 5, 9)
RANKS = (1, 2, 3, 5, 8)
ROOT_SKIPS = (0, 2, 3)
PATTERNS = ("plain", "repeat", "mixed", "plain", "all miss", "inside", "mixed")
# camera kinds: 0..3 are those of table_cases._camera (orbit, eye inside, axis-aligned, grazing a face)
MISS, INSIDE, PARTIAL = 4, 1, 5
CENTRE = np.array([0.5, 0.5, 0.5])


@dataclass
class Case:
    name: str
    mode: str                  # "naive u8" (LAYOUT_AUTO), "naive f16" (LAYOUT_STAGED), "compute" (generate_xor 16^3), "procedural" (no volume)
    W: int
    H: int
    half: bool                 # RGBA16F output (else RGBA32F)
    wire: int                  # WIRE_RGBA / WIRE_RGB
    ts: int
    batches: tuple             # consecutive batches; a batch is a tuple of (kind, camera_blob arguments)
    deals: tuple               # (nranks, root_skip) pairs
    dims: tuple = (24, 24, 24)
    seed: int = 1
    tags: tuple = field(default_factory=tuple)

    @property
    def naive(self):
        return self.mode.startswith("naive")

    @property
    def dt(self):
        return {"naive u8": 1.0, "naive f16": 1.0, "compute": 1.0, "procedural": 3.0}[self.mode]

    @property
    def sequence(self):
        return len(self.batches) > 1

    @property
    def tiles(self):
        return -(-self.W // self.ts) * -(-self.H // self.ts)

    def volume(self, O):
        """What the context is given: a u8 stand-in, an f16 fog, the (density, normals) pair the xor generator makes, or None."""
        if self.mode == "naive u8":
            return O.volume_standin_u8(self.dims, seed=self.seed)
        if self.mode == "naive f16":
            return O.volume_fog_f16(self.dims, seed=self.seed)
        if self.mode == "compute":
            return O.volume_xor(16, 0.0)
        return None

    def cameras(self, O, batch=0):
        return [O.camera_blob(*cam) for _, cam in self.batches[batch]]

    def __repr__(self):
        return (f"Case({self.name}: {self.mode} {self.W}x{self.H} {'rgba16f' if self.half else 'rgba32f'} ts={self.ts} "
                f"wire={'rgb' if self.wire else 'rgba'} batches={[len(b) for b in self.batches]} deals={list(self.deals)})")


# ---- cameras ----

def _miss(O, rng, W, H):
    for _ in range(256):
        cam = _miss_once(O, rng, W, H)
        if cam is not None:
            return cam
    raise AssertionError("no camera misses the box at %d x %d" % (W, H))


def _miss_once(O, rng, W, H):
    """The target far off axis: the whole box lies in front of the eye plane (a corner behind it would switch the silhouette test off and make
    every tile active) and projects clear of the screen by more than 4 pixels (the silhouette test keeps a margin of 2), so that no tile is
    active -- at a 1 x 1 frame that is 9 half-widths off its centre.  Off the left or the top edge: a box beyond the right or bottom edge of
    a frame that is no multiple of the tile size leaves the last column or row of tiles active (their extent reaches past the frame's edge,
    where the clamped silhouette rectangle sits; harmless, they render clear colour)."""
    corners = np.array([[x, y, z, 1.0] for z in (0, 1) for y in (0, 1) for x in (0, 1)])
    zoom, pitch, yaw = float(rng.uniform(1.0, 2.0)), float(rng.uniform(-1.2, 1.2)), float(rng.uniform(0, 6.28))
    # the orientation depends on pitch and yaw alone: moving the target moves the eye with it.  Put the box 30 units from the eye, at a
    # growing angle off the view direction, in a random direction across it
    eye = np.frombuffer(O.camera_blob(zoom, pitch, yaw, tuple(CENTRE), W / H), np.float32)[:3].astype(np.float64)
    view = (CENTRE - eye) / np.linalg.norm(CENTRE - eye)
    across = np.cross(view, rng.normal(size=3))
    across /= np.linalg.norm(across)
    mx, my = 1.0 + 8.0 / W, 1.0 + 8.0 / H
    for deg in range(50, 88):
        t = np.radians(deg)
        shift = CENTRE - eye - 30.0 * (np.cos(t) * view + np.sin(t) * across)
        cam = (zoom, pitch, yaw, tuple(float(v) for v in CENTRE + shift), W / H)
        pv = np.frombuffer(O.camera_blob(*cam), np.float32)[4:20].astype(np.float64).reshape(4, 4)  # column-major: row j is column j
        clip = corners @ pv
        if (clip[:, 3] <= 0.5).any():
            break
        ndc = clip[:, :2] / clip[:, 3:4]
        if (ndc[:, 0] < -mx).all() or (ndc[:, 1] > my).all():
            return cam
    return None


def _partial(rng, W, H, side=None):
    """An orbit that looks past the box: the box covers part of the frame, off its centre (towards `side` of the world's x axis when given)."""
    off = rng.uniform(0.35, 0.8, 3) * rng.choice([-1.0, 1.0], 3)
    if side is not None:
        off[0] = side * abs(off[0])
    return (float(rng.uniform(2.0, 3.2)), float(rng.uniform(-0.6, 0.6)), float(rng.uniform(0, 6.28)), tuple(float(v) for v in CENTRE + off), W / H)


def _cam(O, rng, kind, W, H, naive, side=None):
    """A camera of `kind` for the box [0, 1]^3 of the naive modes; the compute twin's box is [-1, 1]^3 (every tile is active there whatever the
    camera: the kinds only vary the picture)."""
    if kind == MISS and naive:
        cam = _miss(O, rng, W, H)
    elif kind in (PARTIAL, MISS):
        cam = _partial(rng, W, H, side)
    else:
        cam = _camera(rng, kind, W, H)
    if not naive:
        zoom, pitch, yaw, tgt, aspect = cam
        cam = (2.0 * zoom + (0.0 if kind == INSIDE else 1.0), pitch, yaw, tuple(2.0 * (t - 0.5) for t in tgt), aspect)
    return (kind, cam)


def _batch(O, rng, pattern, B, W, H, naive, side=None):
    if pattern == "all miss":
        kinds = [MISS] * B
    elif pattern == "inside":
        kinds = [INSIDE] * B
    elif pattern == "mixed" and B >= 3:
        kinds = ([MISS, INSIDE, PARTIAL, 0, PARTIAL, MISS, 3, PARTIAL, INSIDE] * 2)[:B]
    elif pattern == "partial":
        kinds = [PARTIAL] * B
    else:
        kinds = [(0, 2, 3, PARTIAL, 0, 3, 2, PARTIAL, 0)[k % 9] for k in range(B)]
    cams = [_cam(O, rng, k, W, H, naive, side) for k in kinds]
    if pattern == "repeat" and B >= 2:  # a repeated camera inside the batch (its tables are copied, not computed again)
        cams[B // 2] = cams[B // 2 - 1]
        if B >= 4:
            cams[-1] = cams[0]
    return tuple(cams)


def _deals(i, n=3):
    return tuple((RANKS[(i + 2 * j) % 5], ROOT_SKIPS[(i + j) % 3]) for j in range(n))


@functools.lru_cache(maxsize=None)
def _cases(O):
    rng = np.random.default_rng(SEED)
    cases = []
    for i in range(N_RANDOM):
        W, H = SIZES[i % len(SIZES)]
        mode = MODES[i % len(MODES)]
        B = BATCHES[(2 * i + i // 5) % len(BATCHES)]
        pattern = PATTERNS[(i + i // 7) % len(PATTERNS)]
        dims = tuple(int(v) for v in rng.integers(24, 34, 3)) if mode == "naive u8" else (24, 24, 24)
        cases.append(Case(f"r{i:02d} {pattern}", mode, W, H, i % 2 == 1, (WIRE_RGB, WIRE_RGBA, WIRE_RGB)[i % 3], TILES[i % len(TILES)],
                          (_batch(O, rng, pattern, B, W, H, mode.startswith("naive")),), _deals(i), dims, int(rng.integers(1, 1 << 30)),
                          tags=(pattern,)))
    # one tile of 1024 x 1024 pixels holds the whole frame: 16384 blocks of which one is inside it
    cases.append(Case("tile 1024", "naive u8", 33, 17, True, WIRE_RGB, 1024, (_batch(O, rng, "plain", 1, 33, 17, True),), ((1, 0), (2, 0)), (24, 25, 26), 7))
    # a missing frame, a fully active one and partly active ones in one batch: the clearing strips are sized by n_tiles - min_active, the
    # march by max_active
    cases.append(Case("mixed 97x61", "naive u8", 97, 61, False, WIRE_RGB, 16, (_batch(O, rng, "mixed", 5, 97, 61, True),), ((2, 0), (3, 2), (8, 3)), (33, 24, 29), 11,
                      tags=("mixed",)))
    cases.append(Case("mixed 33x130 staged", "naive f16", 33, 130, True, WIRE_RGBA, 24, (_batch(O, rng, "mixed", 4, 33, 130, True),), ((1, 0), (5, 0), (2, 2)),
                      tags=("mixed",)))
    cases.append(Case("mixed 129x65 ts 8", "naive u8", 129, 65, True, WIRE_RGB, 8, (_batch(O, rng, "mixed", 3, 129, 65, True),), ((3, 0), (2, 3)), (25, 31, 24), 13,
                      tags=("mixed",)))
    cases.append(Case("mixed 120x72 ts 40", "naive u8", 120, 72, False, WIRE_RGBA, 40, (_batch(O, rng, "mixed", 9, 120, 72, True),), ((8, 2), (5, 3)), (28, 28, 33), 17,
                      tags=("mixed",)))
    # every frame misses: no active slot at all (whole frames: only the clearing strips; compact: the early return)
    cases.append(Case("all miss 4", "naive u8", 97, 61, True, WIRE_RGBA, 24, (_batch(O, rng, "all miss", 4, 97, 61, True),), ((1, 0), (3, 0), (2, 2)), (24, 24, 30), 19,
                      tags=("all miss",)))
    cases.append(Case("all miss 1", "naive f16", 7, 5, False, WIRE_RGB, 8, (_batch(O, rng, "all miss", 1, 7, 5, True),), ((1, 0), (2, 0), (5, 3)), tags=("all miss",)))
    # more ranks than active tiles: a frame of one tile dealt to 8, a frame of four tiles with one partly active camera dealt to 8 and 5
    cases.append(Case("one tile, 8 ranks", "naive u8", 8, 8, False, WIRE_RGB, 8, (_batch(O, rng, "plain", 3, 8, 8, True),), ((8, 0), (8, 2), (5, 3), (3, 3)), (24, 24, 24), 23))
    cases.append(Case("four tiles, 8 ranks", "naive u8", 64, 64, True, WIRE_RGBA, 40, (_batch(O, rng, "partial", 4, 64, 64, True),), ((8, 3), (5, 2), (8, 0)), (26, 24, 31), 29))
    cases.append(Case("1x1, 5 ranks", "procedural", 1, 1, True, WIRE_RGB, 16, (_batch(O, rng, "plain", 1, 1, 1, False),), ((5, 0), (2, 2))))
    # sequences for the over un-tile: the box to one side, to the other, a mixed batch, an orbit, the eye inside, the first side again (the
    # last batch has inactive tiles, and shares some with the first: what an un-tile over a stale `prev` would leave unwritten)
    for name, mode, (W, H), half, wire, ts, B, deal, dims, seed in (
            ("seq 97x61", "naive u8", (97, 61), True, WIRE_RGB, 16, 3, (2, 0), (30, 24, 27), 31),
            ("seq 33x130 staged", "naive f16", (33, 130), False, WIRE_RGBA, 8, 1, (1, 0), (24, 24, 24), 37),
            ("seq 129x65", "naive u8", (129, 65), False, WIRE_RGB, 24, 4, (3, 2), (24, 33, 25), 41),
            ("seq 120x72", "naive u8", (120, 72), True, WIRE_RGBA, 40, 5, (2, 3), (27, 27, 24), 43)):
        batches = tuple(_batch(O, rng, p, B, W, H, True, side) for p, side in
                        (("partial", -1.0), ("partial", 1.0), ("mixed" if B >= 3 else "all miss", None), ("plain", None), ("inside", None), ("partial", -1.0)))
        cases.append(Case(name, mode, W, H, half, wire, ts, batches, (deal,), dims, seed, tags=("sequence",)))
    return tuple(cases)


N_CASES = N_RANDOM + 10 + 4


def cases(O):
    """The case list (deterministic: built once from SEED).  O: the oracle module (the tests' `O` fixture), for the camera blobs."""
    out = _cases(O)
    assert len(out) == N_CASES, len(out)
    return out
