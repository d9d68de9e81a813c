"""vk_measure_components restated in numpy from the rule in include/vokselis_hip.h: whole-array operations, one np.bincount or np.add.at
per sum.  Every addend is split so that no array sum leaves the exact range of its dtype (bincount's float64 weights below 2^53, int64
below 2^63), and the pieces are joined as Python ints.  Shares nothing with the library's runs and limbs or with the C restatement's walk.
Output: uint64 [n_regions, 27], the columns of tests/measure_restatement.c."""
import numpy as np

COLS = 27
SCALE = {"u8": 255, "u16": 65535, "f16": 1 << 24}
_U64 = (1 << 64) - 1


def q_of(vol, kind):
    """(q int64, finite bool): the stored texel on the integer scale.  A half times 2^24 is exact in float64."""
    v = np.asarray(vol)
    if kind != "f16":
        return v.astype(np.int64), np.ones(v.shape, bool)
    finite = np.isfinite(v)
    return np.where(finite, np.ldexp(np.where(finite, v, 0).astype(np.float64), 24), 0.0).astype(np.int64), finite


def _exact_sums(ids, values, n):
    """Python ints: per id the sum of the int64 `values` (|v| < 2^62), by bincounts of 24-bit pieces of the magnitude, positives and negatives apart."""
    out = [0] * n
    for sign in (1, -1):
        sel = values * sign > 0
        mag = (values[sel] * sign).astype(np.uint64)
        who = ids[sel]
        for piece in range(3):
            part = ((mag >> np.uint64(24 * piece)) & np.uint64((1 << 24) - 1)).astype(np.float64)   # < 2^24 each: 2^29 of them stay below 2^53
            tot = np.bincount(who, weights=part, minlength=n)
            for k in np.flatnonzero(tot):
                out[k] += sign * (int(tot[k]) << (24 * piece))
    return out


def measure(vol, kind, labels, n_regions):
    """(table uint64 [n_regions, 27], n_foreground)."""
    lab = np.asarray(labels, np.uint32)
    assert lab.shape == np.asarray(vol).shape and (lab.max(initial=0) <= n_regions)
    n = int(n_regions)
    fg = lab != 0
    ids = lab[fg].astype(np.int64) - 1
    z, y, x = (c[fg].astype(np.int64) for c in np.indices(lab.shape))
    nx = lab.shape[2]
    lin = x + nx * (y + lab.shape[1] * z)
    cols = [[0] * n for _ in range(COLS)]
    cols[0] = [int(v) for v in np.bincount(ids, minlength=n)]
    first = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(first, ids, lin)
    cols[1] = [int(f) if m else _U64 for f, m in zip(first, cols[0])]
    for a, c in enumerate((x, y, z)):
        lo, hi = np.full(n, np.iinfo(np.int64).max), np.full(n, -1)
        np.minimum.at(lo, ids, c)
        np.maximum.at(hi, ids, c)
        cols[2 + a] = [int(v) if m else 0 for v, m in zip(lo, cols[0])]
        cols[5 + a] = [int(v) + 1 if m else 0 for v, m in zip(hi, cols[0])]
    for k, t in enumerate((x, y, z, x * x, y * y, z * z, x * y, x * z, y * z)):
        cols[8 + k] = _exact_sums(ids, t, n)
    q, finite = q_of(vol, kind)
    q, finite = q[fg], finite[fg]
    cols[17] = [int(v) for v in np.bincount(ids[~finite], minlength=n)]
    qmin, qmax = np.full(n, np.iinfo(np.int64).max), np.full(n, np.iinfo(np.int64).min)
    np.minimum.at(qmin, ids[finite], q[finite])
    np.maximum.at(qmax, ids[finite], q[finite])
    cols[18], cols[19] = [int(v) & _U64 for v in qmin], [int(v) & _U64 for v in qmax]
    sq = _exact_sums(ids[finite], q[finite], n)
    # q q < 2^80: |q| = h 2^20 + l, q q = h h 2^40 + 2 h l 2^20 + l l, three sums of products below 2^40
    mag = np.abs(q[finite])
    h, l = mag >> 20, mag & ((1 << 20) - 1)
    hh, hl, ll = (_exact_sums(ids[finite], t, n) for t in (h * h, h * l, l * l))
    sqq = [(a << 40) + (b << 21) + c for a, b, c in zip(hh, hl, ll)]
    cols[20], cols[21] = [(v >> 64) & _U64 for v in sq], [v & _U64 for v in sq]
    cols[22], cols[23] = [(v >> 64) & _U64 for v in sqq], [v & _U64 for v in sqq]
    padded = np.pad(lab, 1)   # label 0 around the volume
    core = (slice(1, -1),) * 3
    for a, axis in enumerate((2, 1, 0)):   # faces across x, y, z
        exposed = np.zeros(lab.shape, np.int64)
        for shift in (1, -1):
            exposed += np.roll(padded, shift, axis=axis)[core] != lab
        cols[24 + a] = [int(v) for v in np.bincount(ids, weights=exposed[fg].astype(np.float64), minlength=n)]
    table = np.array([[cols[c][k] for c in range(COLS)] for k in range(n)], dtype=object)
    return (table.astype(np.uint64) if n else np.zeros((0, COLS), np.uint64)), int(fg.sum())
