"""CPU half of the partition fuzz: the case list of tests/partition_cases.py holds what it was built for (so that the GPU module cannot pass
on an empty or friendly list), and the numpy reference of tests/np_partition_reference.py agrees with the library's host functions and with
itself.  vk_tiles_active and vk_partition_slots(_weighted) are pure host arithmetic: they run here through the built library."""
import ctypes as C

import numpy as np

import np_partition_reference as NP
import partition_cases as PC

MODE_ID = {"naive u8": 0, "naive f16": 0, "compute": 1, "procedural": 2}
# bit patterns that must travel untouched: quiet and signalling NaNs with payloads, both infinities, -0, subnormals
EDGE16 = (0x7E00, 0x7C01, 0xFC01, 0xFE55, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x83FF)
EDGE32 = (0x7FC00000, 0x7F800001, 0xFF800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF)


def _active(lib, blob, mode, W, H, ts):
    tx, ty = NP.tiles_xy(W, H, ts)
    act, n = (C.c_ubyte * (tx * ty))(), C.c_uint32()
    assert lib.vk_tiles_active(blob, MODE_ID[mode], W, H, ts, act, C.byref(n)) == 0
    mask = np.frombuffer(act, np.uint8).astype(bool)
    assert n.value == mask.sum()
    return mask


def _batch_masks(lib, O, c, batch=0):
    return np.stack([_active(lib, blob, c.mode, c.W, c.H, c.ts) for blob in c.cameras(O, batch)])


def _orders(rng, masks):
    """A tile order per frame as the library makes them: the active tiles, in some order, in front of the inactive ones."""
    orders = []
    for m in masks:
        on, off = np.nonzero(m)[0], np.nonzero(~m)[0]
        orders.append(np.concatenate([rng.permutation(on), rng.permutation(off)]))
    return orders, masks.sum(axis=1)


def _random_frames(rng, B, H, W, half, wire):
    dt = np.uint16 if half else np.uint32
    f = rng.integers(0, 1 << (16 if half else 32), (B, H, W, 4), dtype=np.uint64).astype(dt)
    edge = np.array(EDGE16 if half else EDGE32, dt)
    m = rng.random(f.shape) < 0.2
    f[m] = rng.choice(edge, int(m.sum()))
    f.reshape(-1)[:len(edge)] = edge[:f.size]  # each pattern at least once where the frame has room
    if wire == NP.WIRE_RGB:
        f[..., 3] = NP.one_bits(dt)
    return f


def test_case_list_holds_what_it_is_built_for(hip_built, O):
    cases = PC.cases(O)
    n_frames = zero = full = mixed = more_ranks = empty_batches = 0
    trans = {gap: np.zeros((2, 2), np.int64) for gap in (1, 2)}
    for c in cases:
        per_batch = [_batch_masks(hip_built, O, c, k) for k in range(len(c.batches))]
        for m, batch in zip(per_batch, c.batches):
            n = m.sum(axis=1)
            n_frames += len(n)
            if c.naive:
                # a camera of the missing kind misses at every frame and tile size, so a batch made of them has no active slot
                assert all(n[j] == 0 for j, (kind, _) in enumerate(batch) if kind == PC.MISS), (c, n.tolist())
                empty_batches += int((n == 0).all())
                zero += int((n == 0).sum())
                full += int((n == c.tiles).sum()) if c.tiles > 1 else 0
                mixed += int(len(n) >= 3 and (n == 0).any() and (n == c.tiles).any() and ((n > 0) & (n < c.tiles)).any())
            else:
                assert (n == c.tiles).all(), c  # the compute twin's box: every tile is active
        most = int(per_batch[0].sum(axis=1).max())
        more_ranks += sum(1 for nr, _ in c.deals if 0 < most < nr)
        if c.sequence:
            # six batches, the last with tiles that are inactive in it and in the first (what an un-tile over a stale `prev` would skip)
            assert (~per_batch[-1] & ~per_batch[0]).sum() > 0 and len(c.batches) == 6, c
            assert len(c.batches) >= 3 and len({len(b) for b in c.batches}) == 1, c
            for gap in (1, 2):
                for i in range(len(per_batch) - gap):
                    was, now = per_batch[i], per_batch[i + gap]
                    for a in (0, 1):
                        for b in (0, 1):
                            trans[gap][a, b] += int(((was == bool(a)) & (now == bool(b))).sum())
    odd_w = np.mean([c.W % 2 for c in cases])
    odd_h = np.mean([c.H % 2 for c in cases])
    print(f"\npartition cases: {len(cases)} cases, {n_frames} frames; {zero} frames with no active tile, {full} with every tile active (of more "
          f"than one), {mixed} mixed batches, {empty_batches} batches in which every frame misses, {more_ranks} (nranks, root_skip) pairs with more ranks than active tiles, odd width {odd_w:.2f}, "
          f"odd height {odd_h:.2f}; transitions [was active][is active] to the next batch {trans[1].tolist()}, to the one after {trans[2].tolist()}")
    assert len(cases) == PC.N_CASES >= 40
    assert zero >= 4 and full >= 4 and mixed >= 3 and more_ranks >= 3, (zero, full, mixed, more_ranks)
    # batches without an active slot on both halves of the list the GPU module walks, with one frame and with several
    for half in (0, 1):
        assert sum(1 for i, c in enumerate(cases) if i % 2 == half and c.naive and "all miss" in c.tags) >= 1, half
    assert {len(c.batches[0]) > 1 for c in cases if c.naive and "all miss" in c.tags} == {False, True} and empty_batches >= 5
    assert trans[1].min() >= 5 and trans[2].min() >= 5, trans
    assert 0.6 <= odd_w <= 0.75 and 0.45 <= odd_h <= 0.6, (odd_w, odd_h)
    # every value of every axis the issue lists is dealt at least once
    assert {c.ts for c in cases} >= {8, 16, 24, 40, 64, 128, 1024} and sum(c.ts == 1024 for c in cases) == 1
    assert {(c.W, c.H) for c in cases} >= {(97, 61), (33, 130), (129, 65), (7, 5), (1, 1), (8, 8), (64, 64), (120, 72)}
    assert {len(c.batches[0]) for c in cases} >= {1, 3, 4, 5, 9}
    assert {nr for c in cases for nr, _ in c.deals} >= {1, 2, 3, 5, 8} and {k for c in cases for nr, k in c.deals if nr > 1} >= {0, 2, 3}
    assert {(c.half, c.wire) for c in cases} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    assert {c.mode for c in cases} == {"naive u8", "naive f16", "compute", "procedural"}
    assert any(len(set(b)) < len(b) for c in cases for b in c.batches), "no batch repeats a camera"
    assert any(c.ts > max(c.W, c.H) for c in cases) and any(k == PC.INSIDE for c in cases for b in c.batches for k, _ in b)
    # the tile order switches to one estimate ray per tile at four frames: both sides are dealt, in compact batches of several ranks
    assert any(len(c.batches[0]) < 4 and c.tiles > 4 for c in cases) and any(len(c.batches[0]) >= 4 and c.tiles > 4 for c in cases)


def test_slot_counts_equal_the_librarys(hip_built, O):
    n, checked = C.c_uint32(), 0
    for c in PC.cases(O):
        for nr in PC.RANKS:
            for k in PC.ROOT_SKIPS:
                want = NP.slot_count(c.tiles, nr, k)
                assert hip_built.vk_partition_slots_weighted(c.W, c.H, c.ts, nr, k, C.byref(n)) == 0 and n.value == want, (c, nr, k, n.value, want)
                if k == 0:
                    assert hip_built.vk_partition_slots(c.W, c.H, c.ts, nr, C.byref(n)) == 0 and n.value == want, (c, nr, n.value, want)
                checked += 1
    # the deal's two statements agree: the round-by-round one of the reference and vokselis_amd.dist's closed forms
    from vokselis_amd import dist as D

    for nr in PC.RANKS:
        for k in PC.ROOT_SKIPS:
            for tiles in (0, 1, 2, nr - 1, nr, nr + 1, 3 * nr - 1, 37, 153):
                rank, slot, rounds = NP.deal(tiles, nr, k)
                kk = k if nr > 1 else 0
                assert rounds == D.deal_rounds(tiles, nr, kk), (tiles, nr, k)
                for q in range(tiles):
                    assert D.deal_owner(q, nr, kk) == (rank[q], slot[q]) and D.deal_pos(int(rank[q]), int(slot[q]), nr, kk) == q, (tiles, nr, k, q)
                assert len({(r, s) for r, s in zip(rank, slot)}) == tiles and (slot < max(rounds, 1)).all()
    assert checked == PC.N_CASES * 15


def test_reference_round_trip_in_both_wire_formats(hip_built, O):
    """Random frames, NaN and inf bit patterns among them, encoded into the ranks' buffers and un-tiled again: the frames come back bit for
    bit on the active tiles, (0, 0, 0, 1) on the others -- for every case's size, tile size and deals, in BOTH wire formats and both widths."""
    from vokselis_amd import dist as D

    rng = np.random.default_rng(PC.SEED + 1)
    runs = 0
    for index, c in enumerate(PC.cases(O)):
        pairs = ((c.half, c.wire),)
        if index % 3 == 0 and c.ts <= 128:  # the other width and wire format at every third case: all four pairs meet every tile size
            pairs += ((not c.half, 1 - c.wire),)
        masks = _batch_masks(hip_built, O, c)
        orders, n_active = _orders(rng, masks)
        B = len(orders)
        for half, wire in pairs:
            frames = _random_frames(rng, B, c.H, c.W, half, wire)
            want = frames.copy()
            want[~NP.tile_pixels(masks, c.W, c.H, c.ts)] = NP.clear_pixel(frames.dtype)
            for nr, k in c.deals:
                slots = NP.slot_count(int(n_active.max()), nr, k) + 1  # (a slot beyond the active ones: never written, never read)
                g = NP.encode(frames, c.ts, orders, n_active, nr, k, wire, slots)
                assert (g[:, slots - 1] == g.dtype.type(0xFFFF if half else 0xFFFFFFFF)).all()
                got = NP.untile(g, c.W, c.H, c.ts, orders, n_active, k, wire)
                assert (got == want).all(), (c, half, wire, nr, k)
                if wire == NP.WIRE_RGBA:  # the package's own statement of the un-tile, given the records as tiles
                    tiles = g.view(np.float16 if half else np.float32).reshape(nr, slots, B, c.ts, c.ts, 4)
                    ref = D.untile_batch_reference(tiles, c.W, c.H, c.ts, orders, n_active, k if nr > 1 else 0)
                    assert (NP.bits(ref) == want).all(), (c, half, nr, k)
                runs += 1
    assert runs >= 3 * 30 + 30


def test_over_untile_equals_the_full_one_along_the_sequences(hip_built, O):
    """Along every sequence, batch i un-tiled over what batch i - 1 (and, with two buffers, batch i - 2) left in the buffer equals its full
    un-tile; over a buffer that holds something else, exactly the tiles inactive then and now keep what was there."""
    rng = np.random.default_rng(PC.SEED + 2)
    seqs = [c for c in PC.cases(O) if c.sequence]
    assert len(seqs) >= 4
    kept = 0
    for c in seqs:
        nr, k = c.deals[0]
        tabs, full = [], []
        for i in range(len(c.batches)):
            masks = _batch_masks(hip_built, O, c, i)
            orders, n_active = _orders(rng, masks)
            frames = _random_frames(rng, len(orders), c.H, c.W, c.half, c.wire)
            g = NP.encode(frames, c.ts, orders, n_active, nr, k, c.wire, NP.slot_count(int(n_active.max()), nr, k))
            tabs.append((masks, orders, n_active, g))
            full.append(NP.untile(g, c.W, c.H, c.ts, orders, n_active, k, c.wire))
        for gap in (1, 2):
            bufs = [None] * gap
            for i, (masks, orders, n_active, g) in enumerate(tabs):
                prev = tabs[i - gap] if i >= gap else None
                out = NP.untile(g, c.W, c.H, c.ts, orders, n_active, k, c.wire, bufs[i % gap],
                                None if prev is None else prev[1], None if prev is None else prev[2])
                assert (out == full[i]).all(), (c, gap, i)
                bufs[i % gap] = out
                if prev is not None:
                    junk = np.full_like(out, 0xFF if not c.half else 0xFFFF) | out.dtype.type(0xFFFFFFFF if not c.half else 0xFFFF)
                    over = NP.untile(g, c.W, c.H, c.ts, orders, n_active, k, c.wire, junk.copy(), prev[1], prev[2])
                    idle = NP.tile_pixels(~prev[0] & ~masks, c.W, c.H, c.ts)
                    assert (over[idle] == junk[idle]).all() and (over[~idle] == full[i][~idle]).all(), (c, gap, i)
                    kept += int(idle.sum())
    assert kept > 0
