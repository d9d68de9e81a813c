"""The code around the march on the MI355X -- the batched launch (vk_render_batch: map_pixel, store_out, clear_inactive_strip), the root's
un-tile (vk_untile, vk_untile_batch, vk_untile_batch_over: untile_batch_kernel) and the host code that sizes and addresses them -- over the
shared fuzz cases (tests/partition_cases.py: odd frame sizes, frames smaller than a tile, cameras that miss the box, more ranks than tiles),
against vk_render's frames bit for bit and against the numpy statement of the deal, the wire records and the un-tile
(tests/np_partition_reference.py).  The CPU suite holds the case list to the conditions it is built for and the reference to the library's
host functions and to itself (tests/test_partition_fuzz_cpu.py).  Every comparison is bitwise except the anchor of a single frame to the
oracle (gpu_helpers.TOL, equal step counts).  Every buffer the library writes starts as 0xFF bytes: what it does not write shows."""
import ctypes as C
import time

import numpy as np
import pytest

import np_partition_reference as NP
import partition_cases as PC
from gpu_helpers import TOL, V, _DevicePtr  # noqa: F401

pytestmark = pytest.mark.gpu

VK_ERR_INVALID = -1


def _mode(V, c):
    return {"naive u8": V.MODE_NAIVE_TRILINEAR, "naive f16": V.MODE_NAIVE_TRILINEAR, "compute": V.MODE_COMPUTE_NEAREST, "procedural": V.MODE_PROCEDURAL}[c.mode]


def _upload_volume(V, O, c, ctx):
    if c.mode == "naive u8":
        V.VolumeTexture(ctx, c.volume(O), layout=V.LAYOUT_AUTO)
    elif c.mode == "naive f16":
        V.VolumeTexture(ctx, c.volume(O), layout=V.LAYOUT_STAGED)
    elif c.mode == "compute":
        V.VolumeTexture.generate_xor(ctx, (16, 16, 16), 0.0)
    else:  # PROCEDURAL reads Uniform.time: pinned to the oracle's default
        ctx.global_uniform.time = 0.0
        V.native.check(ctx.handle, V.native.lib().vk_set_uniform(ctx.handle, ctx.global_uniform.to_bytes()))


def _context(V, O, c, half=None, wire=None):
    half = c.half if half is None else half
    ctx = V.Context(c.W, c.H, backbuffer=(c.W, c.H), out_format=V.OUT_RGBA16F if half else V.OUT_RGBA32F)
    try:
        _upload_volume(V, O, c, ctx)
        ctx.set_wire(c.wire if wire is None else wire)
    except Exception:
        ctx.close()
        raise
    return ctx


def _ff(*shape, half):
    """A device buffer of 0xFF bytes, as integers of the channel's width."""
    import torch

    t = torch.full(shape, -1, dtype=torch.int16 if half else torch.int32, device="cuda")
    torch.cuda.synchronize()  # (torch's stream and the context's do not order each other)
    return t


def _host(t):
    """The buffer's bits on the host (after the library's stream and torch's have drained)."""
    import torch

    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint16 if a.dtype == np.int16 else np.uint32)


def _singles(V, ctx, pipe, cams):
    out = []
    for cam in cams:
        ctx.set_camera_blob(cam)
        pipe.record(ctx)
        out.append(NP.bits(ctx.read_backbuffer()).copy())
    return np.stack(out)


def _tables(V, ctx, c, cams):
    """Per frame: the tile order and the active count, as the single-frame entry points report them for that camera."""
    orders, n_active = [], []
    for cam in cams:
        ctx.set_camera_blob(cam)
        orders.append(ctx.partition_order(c.ts, _mode(V, c)).copy())
        n_active.append(ctx.partition_active(c.ts, 1, _mode(V, c))[0])
    return orders, np.array(n_active)


def _pin_order_rays(ctx, B):
    """Batches of four or more frames order their tiles by one estimate ray per tile, shorter ones and the single-frame calls by a 3 x 3 grid:
    pinned to the batch's own choice, vk_partition_order reports the order the batch deals."""
    ctx.set_param("order_rays", 1 if B >= 4 else 3)


def _gather(buf, act, cap):
    """What the ranks would send, gathered by copies: the contiguous prefix of active slots -- and, where the capacity allows, one slot more,
    which nobody wrote and nobody may read.  A batch with no active slot still needs a buffer to name."""
    import torch

    if act == 0:
        return _ff(16, half=buf.dtype == torch.int16), 0
    n = min(cap, act + 1)
    g = buf[:, :n].contiguous()
    torch.cuda.synchronize()
    return g, n


def _diff(got, want):
    bad = (got != want).any(axis=-1)
    where = tuple(int(v[0]) for v in np.nonzero(bad))
    return f"{int(bad.sum())} pixels differ; first at (frame, y, x) = {where}: got {got[where].tolist()}, want {want[where].tolist()}"


def _report(name, fails):
    for what, msg in fails[:40]:
        print("FAIL", what, msg)
    print(f"{name}: {len(fails)} mismatches")
    assert not fails, f"{name}: {len(fails)} mismatches; first: {fails[0]}"


def _anchor(V, O, c, cam, single, fails):
    """One single frame against the oracle: rendered again into an rgba32f surface with step counts (within TOL, equal counts); the single
    under test is that frame bit for bit -- rounded to nearest even where the case's surface is rgba16f."""
    if c.mode == "procedural":
        ref, rsteps = O.render_procedural(cam, c.W, c.H, dt_scale=c.dt, time=0.0)
    elif c.mode == "compute":
        den, nrm = c.volume(O)
        ref, rsteps, _ = O.render(cam, den, c.W, c.H, mode=O.MODE_COMPUTE_NEAREST, volume2=nrm, dt_scale=c.dt)
    else:
        ref, rsteps, _ = O.render(cam, c.volume(O), c.W, c.H, dt_scale=c.dt)
    ctx = _context(V, O, c, half=False)
    try:
        ctx.set_camera_blob(cam)
        ctx.reset_step_counts()
        V.RaycastPipeline(_mode(V, c), dt_scale=c.dt, flags=V.RENDER_COUNT).record(ctx)
        img, steps = ctx.read_backbuffer(), ctx.read_steps()
    finally:
        ctx.close()
    err = float(np.abs(img - ref).max())
    print(f"anchor {c.name}: max |single - oracle| = {err:.3e}, {int((steps != rsteps).sum())} step counts differ")
    if not (err <= TOL and (steps == rsteps).all()):
        fails.append((c, f"anchor: the single frame is {err:.3e} from the oracle, {int((steps != rsteps).sum())} step counts differ"))
    want = NP.bits(img.astype(np.float16)) if c.half else NP.bits(img)
    if not (single == want).all():
        fails.append((c, "anchor: the single under test is not the frame held to the oracle: " + _diff(single[None], want[None])))


def _run_case(V, O, c, index, fails, stats):
    mode, B, ts, W, H = _mode(V, c), len(c.batches[0]), c.ts, c.W, c.H
    cams = c.cameras(O)
    rec = NP.record_elems(ts, c.wire)
    rng = np.random.default_rng(PC.SEED + 100 + index)
    ctx = _context(V, O, c)
    try:
        pipe = V.RaycastPipeline(mode, dt_scale=c.dt)
        # a. singles
        singles = _singles(V, ctx, pipe, cams)
        if index % 4 == 0:
            _anchor(V, O, c, cams[0], singles[0], fails)
            stats["anchors"] += 1
        # b. whole frames
        frames = _ff(B, H, W, 4, half=c.half)
        V.render_batch(ctx, pipe, cams, frames.data_ptr(), tile_size=ts)
        ctx.sync()
        got = _host(frames)
        if not (got == singles).all():
            fails.append((c, "whole-frame batch: " + _diff(got, singles)))
        # c. compact batches for every deal
        _pin_order_rays(ctx, B)
        orders, n_active = _tables(V, ctx, c, cams)
        stats["frames"] += B
        stats["missing"] += int((n_active == 0).sum())
        for nr, k in c.deals:
            what = (c, f"ranks {nr} root_skip {k}")
            ctx.set_root_skip(k)
            cap = V.partition_slots(W, H, ts, nr, k)
            want_act = NP.slot_count(int(n_active.max()), nr, k)
            buf = _ff(nr, cap, B, rec, half=c.half)
            acts = []
            for r in range(nr):
                bid, act = V.render_batch(ctx, pipe, cams, buf[r].data_ptr(), tile_size=ts, rank=r, nranks=nr, compact=True, slot_capacity=cap)
                acts.append(act)
            ctx.sync()
            if not (len(set(acts)) == 1 and acts[0] == want_act <= cap):
                fails.append((what, f"n_active_slots {acts}, the reference's slot count {want_act}, capacity {cap}"))
                continue
            act = acts[0]
            stats["more ranks"] += int(0 < n_active.max() < nr)
            stats["batches without an active slot"] += int(act == 0)
            host = _host(buf)
            decoded = NP.untile(host, W, H, ts, orders, n_active, k, c.wire)
            if not (decoded == singles).all():
                fails.append((what, "ranks' buffers decoded by the reference: " + _diff(decoded, singles)))
            # ... and nothing else was written: records of inactive positions, pixels of a record beyond the frame's edge, slots beyond the active ones
            records = NP.encode(singles, ts, orders, n_active, nr, k, c.wire, cap)
            if not (host == records).all():
                fails.append((what, f"{int((host != records).sum())} elements of the ranks' buffers differ from the reference's records (0xFF where nobody writes)"))
            g, n = _gather(buf, act, cap)
            frames = _ff(B, H, W, 4, half=c.half)
            V.untile_batch(ctx, bid, g.data_ptr(), n, frames.data_ptr())
            ctx.sync()
            got = _host(frames)
            if not (got == singles).all():
                fails.append((what, "vk_untile_batch: " + _diff(got, singles)))
            stats["deals"] += 1
        # d. peer-direct: the ranks, in a shuffled order, write their tiles at their place in one set of whole frames
        multi = [d for d in c.deals if d[0] > 1]
        if multi:
            nr, k = multi[index % len(multi)]
            ctx.set_root_skip(k)
            frames = _ff(B, H, W, 4, half=c.half)
            for r in rng.permutation(nr):
                V.render_batch(ctx, pipe, cams, frames.data_ptr(), tile_size=ts, rank=int(r), nranks=nr)
            ctx.sync()
            got = _host(frames)
            if not (got == singles).all():
                fails.append(((c, f"peer-direct, ranks {nr} root_skip {k}"), _diff(got, singles)))
            stats["peer-direct root_skip %s" % ("0" if k == 0 else ">= 2")] += 1
        ctx.set_root_skip(0)
    finally:
        ctx.close()


def _run_cases(V, O, name, picked):
    from collections import Counter

    start = time.perf_counter()
    fails, stats = [], Counter()
    for index, c in picked:
        t0 = time.perf_counter()
        _run_case(V, O, c, index, fails, stats)
        stats["slowest case, ms"] = max(stats["slowest case, ms"], int(1e3 * (time.perf_counter() - t0)))
    print(f"\n{name}: {len(picked)} cases, {dict(stats)}, {time.perf_counter() - start:.1f} s")
    _report(name, fails)
    return stats


def test_batches_equal_singles_first_half(V, O):
    picked = [(i, c) for i, c in enumerate(PC.cases(O)) if i % 2 == 0]
    stats = _run_cases(V, O, "partition fuzz, even cases", picked)
    assert stats["anchors"] >= 10 and stats["deals"] >= 50 and stats["missing"] >= 4 and stats["batches without an active slot"] >= 1


def test_batches_equal_singles_second_half(V, O):
    picked = [(i, c) for i, c in enumerate(PC.cases(O)) if i % 2 == 1]
    stats = _run_cases(V, O, "partition fuzz, odd cases", picked)
    assert stats["deals"] >= 50 and stats["missing"] >= 4 and stats["more ranks"] >= 3 and stats["batches without an active slot"] >= 1
    assert stats["peer-direct root_skip 0"] + stats["peer-direct root_skip >= 2"] >= 6 and stats["peer-direct root_skip 0"] >= 2 and stats["peer-direct root_skip >= 2"] >= 2


def test_untile_over_along_the_sequences(V, O):
    """vk_untile_batch_over along runs of batches of one shape: batch i over what batch i - 1 left in the buffer, and -- two buffers in turn, as
    BatchTileRenderer drives it -- over what batch i - 2 left; then over a buffer of 0xFF bytes with the same `prev`, where exactly the tiles
    inactive then and now keep their 0xFF (the skip under test ran, and ran nowhere else); an unusable `prev` is a full un-tile."""
    start = time.perf_counter()
    fails, kept, calls, stale = [], 0, 0, 0
    seqs = [c for c in PC.cases(O) if c.sequence]
    assert len(seqs) >= 4
    for c in seqs:
        mode, B, ts, W, H = _mode(V, c), len(c.batches[0]), c.ts, c.W, c.H
        nr, k = c.deals[0]
        rec = NP.record_elems(ts, c.wire)
        cap = V.partition_slots(W, H, ts, nr, k)
        ctx = _context(V, O, c)
        peer = _context(V, O, c) if nr > 1 else None  # (a batch id per vk_render_batch call, four held: the root's context renders the root's share only)
        try:
            pipe = V.RaycastPipeline(mode, dt_scale=c.dt)
            for x in (ctx, peer):
                if x is not None:
                    x.set_root_skip(k)
                    _pin_order_rays(x, B)
            bids, tabs = [], []
            chain1, chain2 = _ff(B, H, W, 4, half=c.half), [_ff(B, H, W, 4, half=c.half) for _ in range(2)]
            for i in range(len(c.batches)):
                cams = c.cameras(O, i)
                singles = _singles(V, ctx, pipe, cams)
                orders, n_active = _tables(V, ctx, c, cams)
                buf = _ff(nr, cap, B, rec, half=c.half)
                bid, act = V.render_batch(ctx, pipe, cams, buf[0].data_ptr(), tile_size=ts, rank=0, nranks=nr, compact=True, slot_capacity=cap)
                for r in range(1, nr):
                    _, act_r = V.render_batch(peer, pipe, cams, buf[r].data_ptr(), tile_size=ts, rank=r, nranks=nr, compact=True, slot_capacity=cap)
                    assert act_r == act
                    peer.sync()
                ctx.sync()
                g, n = _gather(buf, act, cap)
                host_g = _host(g).reshape(nr, n, B, rec) if n else np.zeros((nr, 0, B, rec), np.uint16 if c.half else np.uint32)
                masks = NP.active_masks(orders, n_active, c.tiles)
                bids.append(bid)
                tabs.append((orders, n_active, masks))
                for label, out, gap in (("over the batch before", chain1, 1), ("over the batch before last", chain2[i % 2], 2)):
                    prev = bids[i - gap] if i >= gap else 0
                    V.untile_batch(ctx, bid, g.data_ptr(), n, out.data_ptr(), prev_batch_id=prev)
                    ctx.sync()
                    calls += 1
                    got = _host(out)
                    if not (got == singles).all():
                        fails.append(((c, f"batch {i} {label}"), _diff(got, singles)))
                    if i >= gap:  # the same call on a buffer that does NOT hold what `prev` names
                        junk = _ff(B, H, W, 4, half=c.half)
                        V.untile_batch(ctx, bid, g.data_ptr(), n, junk.data_ptr(), prev_batch_id=prev)
                        ctx.sync()
                        got = _host(junk)
                        po, pn, pm = tabs[i - gap]
                        want = NP.untile(host_g, W, H, ts, orders, n_active, k, c.wire, np.full_like(singles, ~singles.dtype.type(0)), po, pn)
                        idle = NP.tile_pixels(~pm & ~masks, W, H, ts)
                        assert (want[idle] == ~singles.dtype.type(0)).all() and (want[~idle] == singles[~idle]).all()
                        if not (got == want).all():
                            fails.append(((c, f"batch {i} {label}, on 0xFF bytes"), _diff(got, want)))
                        kept += int(idle.sum())
            # An unusable prev -- five batches old, a batch of another frame count, an id never issued -- is a full un-tile.  The current batch
            # is the sequence's last: it has inactive tiles, and shares some with the batch of five ago (its first) and with the batch of
            # another frame count (its own cameras and one more), so honouring either would leave 0xFF behind; so would skipping on an unknown id.
            more = cams + [cams[0]]
            other = _ff(cap, B + 1, rec, half=c.half)
            bid_other, _ = V.render_batch(ctx, pipe, more, other.data_ptr(), tile_size=ts, rank=0, nranks=nr, compact=True, slot_capacity=cap)
            for label, prev, was in (("five batches old", bids[-1] - 5, tabs[0][2]), ("another frame count", bid_other, masks), ("never issued", bid_other + 1000, masks)):
                assert prev > 0 and (prev == bids[0]) == (label == "five batches old")
                at_stake = int(NP.tile_pixels(~was & ~masks, W, H, ts).sum())
                assert at_stake > 0, (c, label)
                stale += at_stake
                junk = _ff(B, H, W, 4, half=c.half)
                V.untile_batch(ctx, bid, g.data_ptr(), n, junk.data_ptr(), prev_batch_id=prev)
                ctx.sync()
                calls += 1
                got = _host(junk)
                if not (got == singles).all():
                    fails.append(((c, f"prev {label}"), _diff(got, singles)))
        finally:
            ctx.close()
            if peer is not None:
                peer.close()
    print(f"\nover un-tile: {len(seqs)} sequences, {calls} un-tiles, {kept} pixels kept their 0xFF, {stale} pixels that a wrongly honoured prev would have left 0xFF, {time.perf_counter() - start:.1f} s")
    _report("vk_untile_batch_over", fails)
    assert kept > 0 and stale > 0


def _backbuffer_ff(V, ctx, half):
    """0xFF bytes into the backbuffer through the pointer vk_backbuffer_info returns."""
    import torch

    w, h, fmt, ptr = C.c_uint32(), C.c_uint32(), C.c_int(), C.c_void_p()
    V.native.check(ctx.handle, V.native.lib().vk_backbuffer_info(ctx.handle, C.byref(w), C.byref(h), C.byref(fmt), C.byref(ptr)))
    ctx.sync()
    torch.as_tensor(_DevicePtr(ptr.value, (h.value, w.value, 4), "<i2" if half else "<i4"), device="cuda").fill_(-1)
    torch.cuda.synchronize()


def _other_cameras(O, c, cams):
    """Cameras to change to after a partition: the batch's other cameras, an eye inside the box (every tile active), the box off to a side, the box small in the frame's centre."""
    s, o = (1.0, 0.0) if c.naive else (2.0, -1.0)  # (the compute twin's box is [-1, 1]^3)
    inside = O.camera_blob(0.2 * s, 0.3, 1.0, (0.5 * s + o,) * 3, c.W / c.H)
    aside = O.camera_blob(2.6 * s, 0.3, 1.0, (1.1 * s + o, 1.0 * s + o, 0.0 * s + o), c.W / c.H)
    far = O.camera_blob(9.0 * s, 0.3, 1.0, (0.5 * s + o,) * 3, c.W / c.H)
    return [cam for cam in cams[1:] if cam != cams[0]] + [inside, aside, far]


def test_single_frame_partition_and_untile_at_odd_sizes(V, O):
    """vk_render_partition + vk_untile on the odd-sized cases, in both wire formats, into a backbuffer of 0xFF bytes; once more with the camera
    changed (and no new partition) between the two calls: the un-tile follows the LAST partition call, the frame is the old camera's."""
    start = time.perf_counter()
    fails, runs, differ = [], 0, 0
    lib = V.native.lib()
    odd = [c for c in PC.cases(O) if (c.W % 2 or c.H % 2) and not c.sequence and c.ts <= 128]
    assert len(odd) >= 20
    for index, c in enumerate(odd):
        mode, ts, W, H = _mode(V, c), c.ts, c.W, c.H
        cams = c.cameras(O)
        nr, k = c.deals[index % len(c.deals)]
        ctx = _context(V, O, c)
        try:
            pipe = V.RaycastPipeline(mode, dt_scale=c.dt)
            single = _singles(V, ctx, pipe, [cams[0]])[0]
            # the camera to change to: the first of the candidates whose tile tables (order, active count) differ from the old camera's, so
            # that an un-tile that followed the camera uploaded since would scatter the tiles wrongly or clear marched ones
            other, (old_orders, old_active) = None, _tables(V, ctx, c, [cams[0]])
            for cand in _other_cameras(O, c, cams):
                orders, n_active = _tables(V, ctx, c, [cand])
                if n_active[0] != old_active[0] or (orders[0] != old_orders[0]).any():
                    other = cand
                    break
            differ += other is not None
            if other is None:
                other = _other_cameras(O, c, cams)[0]
            ctx.set_root_skip(k)
            cap = V.partition_slots(W, H, ts, nr, k)
            for wire, change in ((V.WIRE_RGBA, False), (V.WIRE_RGB, False), (c.wire, True)):
                ctx.set_wire(wire)
                ctx.set_camera_blob(cams[0])
                gathered = _ff(nr, cap, NP.record_elems(ts, wire), half=c.half)
                for r in range(nr):
                    pipe.record_partition(ctx, ts, r, nr, gathered[r].data_ptr())
                _backbuffer_ff(V, ctx, c.half)
                if change:
                    ctx.set_camera_blob(other)
                V.native.check(ctx.handle, lib.vk_untile(ctx.handle, C.c_void_p(gathered.data_ptr()), ts, nr, cap))
                got = NP.bits(ctx.read_backbuffer())
                runs += 1
                if not (got == single).all():
                    fails.append(((c, f"ranks {nr} root_skip {k} wire {wire}" + (", camera changed before the un-tile" if change else "")), _diff(got[None], single[None])))
                # the ranks' buffers hold the reference's records of that frame
                orders, n_active = _tables(V, ctx, c, [cams[0]])
                host = _host(gathered).reshape(nr, cap, 1, -1)
                if not (host == NP.encode(single[None], ts, orders, n_active, nr, k, wire, cap)).all():
                    fails.append(((c, f"ranks {nr} root_skip {k} wire {wire}"), "the ranks' buffers differ from the reference's records"))
        finally:
            ctx.close()
    several = sum(1 for c in odd if c.naive and c.tiles > 1)
    print(f"\nsingle-frame partition + un-tile: {len(odd)} cases, {runs} runs, the camera changed to has other tile tables in {differ} cases "
          f"({several} naive cases have more than one tile), {time.perf_counter() - start:.1f} s")
    _report("vk_render_partition + vk_untile", fails)
    # a frame of several tiles under the naive modes' silhouette test: an eye inside the box, the box off to a side or small in the centre changes the active set
    assert differ >= several >= 10, (differ, several)


def test_untile_batch_refusals(V, O):
    """A batch id whose tiles the context no longer describes is refused -- after vk_backbuffer_resize, after a new volume, five batches on --
    and the next batch on the same context works."""
    start = time.perf_counter()
    lib = V.native.lib()
    c = next(c for c in PC.cases(O) if c.name == "mixed 97x61")
    mode, B, ts, W, H = _mode(V, c), len(c.batches[0]), c.ts, c.W, c.H
    cams = c.cameras(O)
    rec = NP.record_elems(ts, c.wire)
    cap = V.partition_slots(W, H, ts, 1)
    ctx = _context(V, O, c)
    try:
        pipe = V.RaycastPipeline(mode, dt_scale=c.dt)
        singles = _singles(V, ctx, pipe, cams)

        def batch():
            buf = _ff(1, cap, B, rec, half=c.half)
            bid, act = V.render_batch(ctx, pipe, cams, buf.data_ptr(), tile_size=ts, compact=True, slot_capacity=cap)
            ctx.sync()
            return bid, act, buf

        def untile(bid, act, buf):
            frames = _ff(B, H, W, 4, half=c.half)
            rc = lib.vk_untile_batch(ctx.handle, bid, C.c_void_p(buf.data_ptr()), cap, C.c_void_p(frames.data_ptr()))
            ctx.sync()
            return rc, _host(frames)

        def works():
            rc, got = untile(*batch())
            assert rc == V.native.VK_OK and (got == singles).all()

        works()
        held = batch()
        ctx.resize_backbuffer(W, H)
        rc, got = untile(*held)
        assert rc == VK_ERR_INVALID and (got == ~got.dtype.type(0)).all(), "un-tiled a batch dealt before vk_backbuffer_resize"
        works()
        held = batch()
        _upload_volume(V, O, c, ctx)
        rc, got = untile(*held)
        assert rc == VK_ERR_INVALID and (got == ~got.dtype.type(0)).all(), "un-tiled a batch dealt for the previous volume"
        works()
        held = batch()
        for _ in range(3):
            batch()
        rc, got = untile(*held)  # three batches on: still held
        assert rc == V.native.VK_OK and (got == singles).all()
        batch()
        batch()
        rc, got = untile(*held)
        assert rc == VK_ERR_INVALID and (got == ~got.dtype.type(0)).all(), "un-tiled a batch of five batches ago"
        works()
    finally:
        ctx.close()
    print(f"\nrefusals: {time.perf_counter() - start:.1f} s")
