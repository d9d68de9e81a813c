"""A plain numpy statement of what surrounds the march in a partitioned frame: the deal of the tile order's positions over ranks, the
compact record of a tile in both wire formats, the root's un-tile and its "over" form (include/vokselis_hip.h: vk_partition_root_skip,
vk_partition_wire, vk_render_batch, vk_untile_batch, vk_untile_batch_over).  Written from the header's words, not from the kernels' index
arithmetic; pixels travel as unsigned integers of the channel's width, so that NaN payloads and infinities are moved and compared as bits.

Layouts:
    frames     [B][H][W][4]
    gathered   [nranks][n_slots][B][record]    one rank's part is what vk_render_batch(compact) writes: [slot][frame][record]
    record     VK_WIRE_RGBA: [ts][ts][4];  VK_WIRE_RGB: ts*ts (r, g) pairs followed by ts*ts b values (alpha is 1)
The pixels of a record that lie outside the frame (tiles on its right and bottom edges) are never written, nor are records of inactive
positions: they keep whatever the buffer held (`fill`)."""
from __future__ import annotations

import numpy as np

from vokselis_amd import dist as D

WIRE_RGBA, WIRE_RGB = 0, 1


def bits(a: np.ndarray) -> np.ndarray:
    """A float16 / float32 array as the unsigned integers of its bit patterns (integers pass through)."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def one_bits(dtype) -> int:
    """1.0 in the channel's format."""
    return 0x3C00 if np.dtype(dtype).itemsize == 2 else 0x3F800000


def clear_pixel(dtype) -> np.ndarray:
    """LoadOp::Clear(BLACK) = (0, 0, 0, 1)."""
    return np.array([0, 0, 0, one_bits(dtype)], dtype)


def record_elems(ts: int, wire: int) -> int:
    return ts * ts * (3 if wire == WIRE_RGB else 4)


# ---- the deal ----

def deal(n_positions: int, nranks: int, root_skip: int = 0):
    """Positions 0 .. n_positions - 1 dealt in rounds, one position per rank and round, rank 0 first; with root_skip = k >= 2 (and more than
    one rank) rank 0 sits out every k-th round.  A rank's slots count the rounds it took part in.  Returns (rank[pos], slot[pos], rounds): the
    number of rounds is the slot count of a rank that never sits out, which is what every rank's buffer is sized by."""
    k = root_skip if nranks > 1 else 0
    rank, slot = np.empty(n_positions, np.int64), np.empty(n_positions, np.int64)
    taken = [0] * nranks
    pos = rnd = 0
    while pos < n_positions:
        for r in range(nranks):
            if r == 0 and k >= 2 and rnd % k == k - 1:
                continue
            if pos < n_positions:
                rank[pos], slot[pos] = r, taken[r]
                pos += 1
            taken[r] += 1
        rnd += 1
    return rank, slot, rnd


def slot_count(n_positions: int, nranks: int, root_skip: int = 0) -> int:
    return deal(n_positions, nranks, root_skip)[2]


def tiles_xy(W: int, H: int, ts: int):
    return -(-W // ts), -(-H // ts)


# ---- records ----

def encode_record(tile: np.ndarray, wire: int) -> np.ndarray:
    """[ts][ts][4] -> the flat record."""
    if wire == WIRE_RGB:
        return np.concatenate([tile[..., :2].reshape(-1), tile[..., 2].reshape(-1)])
    return tile.reshape(-1)


def decode_record(rec: np.ndarray, ts: int, wire: int) -> np.ndarray:
    """The flat record -> [ts][ts][4]; a VK_WIRE_RGB record carries no alpha: it is 1."""
    if wire == WIRE_RGB:
        out = np.empty((ts, ts, 4), rec.dtype)
        out[..., :2] = rec[:2 * ts * ts].reshape(ts, ts, 2)
        out[..., 2] = rec[2 * ts * ts:].reshape(ts, ts)
        out[..., 3] = one_bits(rec.dtype)
        return out
    return rec.reshape(ts, ts, 4)


def encode(frames: np.ndarray, ts: int, orders, n_active, nranks: int, root_skip: int, wire: int, n_slots: int, fill: int = 0xFF) -> np.ndarray:
    """The ranks' compact buffers of a batch, [nranks][n_slots][B][record], every byte nobody writes holding `fill`.  orders[b]: position ->
    row-major tile id of frame b; n_active[b]: its leading active positions, the only ones marched."""
    frames = bits(frames)
    B, H, W, _ = frames.shape
    tx, _ = tiles_xy(W, H, ts)
    filler = np.frombuffer(bytes([fill]) * frames.dtype.itemsize, frames.dtype)[0]
    out = np.full((nranks, n_slots, B, record_elems(ts, wire)), filler, frames.dtype)
    for b in range(B):
        rank, slot, rounds = deal(int(n_active[b]), nranks, root_skip)
        assert rounds <= n_slots, (rounds, n_slots)
        for q in range(int(n_active[b])):
            t = int(orders[b][q])
            y0, x0 = (t // tx) * ts, (t % tx) * ts
            tile = np.full((ts, ts, 4), filler, frames.dtype)
            part = frames[b, y0:y0 + ts, x0:x0 + ts]
            tile[:part.shape[0], :part.shape[1]] = part
            if wire == WIRE_RGB:  # the record has no alpha to leave unwritten
                assert (part[..., 3] == one_bits(frames.dtype)).all(), "VK_WIRE_RGB carries frames whose alpha is 1"
            out[rank[q], slot[q], b] = encode_record(tile, wire)
    return out


# ---- the un-tile ----

def untile(gathered: np.ndarray, W: int, H: int, ts: int, orders, n_active, root_skip: int, wire: int, out: np.ndarray | None = None,
           prev_orders=None, prev_n_active=None) -> np.ndarray:
    """gathered [nranks][n_slots][B][record] -> frames [B][H][W][4] of the same integer type.  Tiles at positions >= n_active[b] of frame b's
    order are cleared to (0, 0, 0, 1).  The over form: `out` still holds what un-tiling an earlier batch (prev_orders, prev_n_active) left
    there; a tile that was inactive in that batch's frame b and is inactive now is not written.  The result then equals the full un-tile
    whenever that word about `out` is true."""
    gathered = bits(gathered)
    nranks, _, B, _ = gathered.shape
    tx, ty = tiles_xy(W, H, ts)
    if out is None:
        assert prev_orders is None
        out = np.zeros((B, H, W, 4), gathered.dtype)
    assert out.shape == (B, H, W, 4) and out.dtype == gathered.dtype
    world = nranks
    for b in range(B):
        pos = np.argsort(np.asarray(orders[b]))  # tile id -> position
        ppos = None if prev_orders is None else np.argsort(np.asarray(prev_orders[b]))
        for t in range(tx * ty):
            y0, x0 = (t // tx) * ts, (t % tx) * ts
            h, w = min(ts, H - y0), min(ts, W - x0)
            q = int(pos[t])
            if q >= int(n_active[b]):
                if ppos is not None and int(ppos[t]) >= int(prev_n_active[b]):
                    continue
                out[b, y0:y0 + h, x0:x0 + w] = clear_pixel(gathered.dtype)
            else:
                r, sl = D.deal_owner(q, world, root_skip if world > 1 else 0)
                out[b, y0:y0 + h, x0:x0 + w] = decode_record(gathered[r, sl, b], ts, wire)[:h, :w]
    return out


def active_masks(orders, n_active, n_tiles: int) -> np.ndarray:
    """[B][n_tiles] bool: which tiles of each frame are active."""
    m = np.zeros((len(orders), n_tiles), bool)
    for b, (o, n) in enumerate(zip(orders, n_active)):
        m[b, np.asarray(o)[:int(n)]] = True
    return m


def tile_pixels(mask_tiles: np.ndarray, W: int, H: int, ts: int) -> np.ndarray:
    """A per-tile flag [..., n_tiles] spread over the pixels: [..., H, W]."""
    tx, ty = tiles_xy(W, H, ts)
    m = mask_tiles.reshape(mask_tiles.shape[:-1] + (ty, tx))
    return np.repeat(np.repeat(m, ts, axis=-2), ts, axis=-1)[..., :H, :W]
