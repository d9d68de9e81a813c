"""Cases for the batched fixed-point loop the split, geodesic and skeleton passes share (PassCall::iterate): the
host enqueues B rounds, reads their counts and stops at the first round that changed nothing.  Each case needs a chosen number of rounds
around a batch boundary -- B - 1, B, B + 1, 2 B, with B read from the pass's header -- and the skeleton also meets its iteration budget
inside a batch, on a batch's last iteration and beyond convergence.  u8, LINEAR, at most 70 x 20 x 12 voxels, and every shape spans
the tile border at x = 32, so that tile stamps cross it inside a batch.  Built from the passes' own Case tuples: their helpers run them.

What sets the count:
  split     a 5^3 block whose core survives the erosion at radius 1, and a bar one voxel thick on it, which does not: the growth
            labels one voxel of the bar per round, so the bar's length is the number of rounds that label something.
  geodesic  a corridor one voxel wide that snakes across the tile border, from a seed at its start.  A tile sees its neighbour's words
            of the launch before, so the front gets one tile crossing further per round: with c crossings on the way to the far end,
            round c + 1 is the last that lowers a word.  Its first voxel lies on the border it crossed and wakes the tile behind it,
            which round c + 2 visits and leaves as it was: c + 2 rounds visit a tile, and round c + 2 is the one that wakes nothing.
  skeleton  a block 66 long: in CURVE mode every iteration peels one layer off each side, so its cross-section sets the iterations."""
import math
import os
import re

import numpy as np

import geo_cases as GC
import skel_cases as KC
import split_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (70, 20, 12)  # x, y, z: three tiles of 32 x 16 x 8 along x, two along y and z


def batch(name):
    """B of a pass (kSplitBatch, kGeoBatch, kSkelBatch) from its header."""
    stem = {"kSplitBatch": "vk_split.hpp", "kGeoBatch": "vk_geo.hpp", "kSkelBatch": "vk_skel.hpp"}[name]
    src = open(os.path.join(ROOT, "vokselis_amd", "csrc", stem)).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, src).group(1))


def counts(b):
    return (b - 1, b, b + 1, 2 * b)


def _empty():
    return np.zeros(DIMS[::-1], np.uint8)


# ---- split --------------------------------------------------------------------------------------------------------------------------
def split_case(rounds):
    v = _empty()
    v[2:7, 2:7, 24:29] = 255             # the block: its 3^3 core is the marker
    v[4, 4, 29:29 + rounds] = 255        # the bar, across x = 32 from its fourth voxel on
    return SC.Case(f"fixed point, split, {rounds} rounds", f"fp split {rounds}", v, "u8", 0.5, math.inf, 6, None, None, (1, 1, 1), 1.0, 0.0)


def split_cases():
    return [(r, split_case(r)) for r in counts(batch("kSplitBatch"))]


# ---- geodesic -----------------------------------------------------------------------------------------------------------------------
def snake(n_rows, last):
    """A corridor of n_rows rows along x over x = 28 .. 36, joined at alternating ends, row after row in y and then in z; the last row
    is `last` voxels long.  (volume, seed, far end)"""
    v = _empty()
    rows = [(y, z) for z in (1, 3, 5, 7, 9) for y in (range(1, 19, 2) if (z // 2) % 2 == 0 else range(17, 0, -2))]
    xa, xb, right, end = 28, 36, True, None
    for i, (y, z) in enumerate(rows[:n_rows]):
        final = i == n_rows - 1
        xs = range(xa, xa + last if final else xb + 1) if right else range(xb, xb - last if final else xa - 1, -1)
        for x in xs:
            v[z, y, x] = 255
        end = xs[-1]
        if not final:
            y2, z2 = rows[i + 1]
            v[(z + z2) // 2, (y + y2) // 2, end] = 255
        right = not right
    y0, z0 = rows[0]
    y1, z1 = rows[n_rows - 1]
    return v, (xa, y0, z0), (end, y1, z1)


def geo_case(n_rows, last):
    v, seed, goal = snake(n_rows, last)
    c = GC.Case(f"fixed point, geodesic, {n_rows} rows, the last {last} long", f"fp geo {n_rows} {last}", v, "u8", 0.5, math.inf, 6, (1, 1, 1), 0, 0, (seed,), 0.0, 0.0, 0.0, None, None)
    return c, goal


# rounds that visit a tile -> (rows, length of the last row): the corridor's tile crossings are that number less 2 (test_fixed_point_cpu.py holds it)
GEO_SHAPES = {7: (6, 3), 8: (6, 9), 9: (7, 9), 16: (13, 3)}


def geo_cases():
    return [(r,) + geo_case(*GEO_SHAPES[r]) for r in counts(batch("kGeoBatch"))]


# ---- skeleton -----------------------------------------------------------------------------------------------------------------------
SKEL_SECTIONS = {3: (7, 7), 4: (9, 9), 5: (10, 10), 8: (19, 11)}  # iterations that delete something -> the block's extent along y and z


def skel_case(iterations, max_iterations=0):
    ty, tz = SKEL_SECTIONS[iterations]
    v = _empty()
    y0, z0 = (DIMS[1] - ty) // 2, (DIMS[2] - tz) // 2
    v[z0:z0 + tz, y0:y0 + ty, 2:68] = 255
    stop = f", at most {max_iterations}" if max_iterations else ""
    return KC.Case(f"fixed point, skeleton, {iterations} iterations{stop}", f"fp skel {iterations}", v, "u8", 0.5, math.inf, KC.CURVE, max_iterations, None, 0.0, None, None)


def skel_cases():
    """(iterations to convergence, max_iterations, case)"""
    b = batch("kSkelBatch")
    out = [(i, 0, skel_case(i)) for i in counts(b)]
    # the budget against the 2 B case: inside the second batch, on the first batch's last iteration, on the second's, and beyond convergence
    return out + [(2 * b, m, skel_case(2 * b, m)) for m in (b + 2, b, 2 * b, 5 * b)]
