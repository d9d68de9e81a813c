"""The C oracle's present pass (oracle/vokselis_oracle.c: vo_present) against the float64 specification (tests/np_present_reference.py)
over the shared fuzz cases (tests/present_cases.py), under the one comparison rule: a byte equals floor(q + 0.5), or either neighbour where
q + 0.5 lies within DELTA of an integer.  The GPU suite (tests/test_present_fuzz_gpu.py) holds vk_present, the fused epilogue and
vk_capture_frame to the same reference over the same list.

Also here, so that the GPU module cannot hide behind them: the list covers every class it claims (inf, NaN, negative, beyond-overflow and
zero-weight-next-to-non-finite samples; one sign per channel wherever a case resamples; magnitudes <= 1e30); DELTA is four times the measured
f32 error of the kernel's operation sequence; undecided bytes are at most 0.5 % of any case of 1000 bytes or more and of the total, and the
boundary case has none; the tone map is monotone over the non-negative f16 values and ends at 255; and the formula the pass had before it was
extended by its limits (inf / inf = NaN -> 0) fails the beyond-overflow values under this rule: the test bites."""
import numpy as np

import np_present_reference as P
import present_cases as PC


def _q(case):
    return P.present_q(case.bb, case.w, case.h)


def test_oracle_present_against_the_reference(O):
    fails, worst, total = [], 0.0, 0
    for c in PC.cases():
        got = O.present(c.bb.astype(np.float32), c.w, c.h)
        q = _q(c)
        wrong, und = P.judge(got, q, PC.DELTA)
        total += got.size
        worst = max(worst, float(np.abs(got.astype(np.float64) - q)[~und].max()))
        if wrong.any():
            y, x, ch = (int(v[0]) for v in np.nonzero(wrong))
            fails.append((c, int(wrong.sum()), f"first at ({x}, {y}) channel {ch}: byte {got[y, x, ch]}, q = {q[y, x, ch]!r}"))
    print(f"\npresent fuzz (oracle): {len(PC.cases())} cases, {total} bytes, largest |byte - q| outside the undecided band {worst:.6f}")
    for f in fails[:20]:
        print("FAIL", *f)
    assert worst <= 0.5 + PC.DELTA
    assert not fails, f"{len(fails)} cases with wrong bytes; first: {fails[0]}"


def test_case_list_covers_what_it_claims():
    cases = PC.cases()
    assert len(cases) == PC.N_CASES
    n_over, d_over = PC.overflow_points()
    assert 1.16e19 < n_over < 1.17e19 and 1.18e19 < d_over < 1.19e19
    counts = dict(inf=0, nan=0, negative=0, beyond=0, zero_weight_by_nonfinite=0, zero_weight_nan_neighbour=0)
    for c in cases:
        with np.errstate(invalid="ignore"):
            v64 = c.bb.astype(np.float64)
        assert np.abs(v64[np.isfinite(v64)]).max(initial=0.0) <= float(np.float32(1e30)), c
        if c.resamples:
            assert PC.one_sign(c), c
        s = P.sample(c.bb, c.w, c.h)
        counts["inf"] += int(np.isinf(s).sum())
        counts["nan"] += int(np.isnan(s).sum())
        counts["negative"] += int((s < 0).sum())
        counts["beyond"] += int((np.abs(s[..., :3]) >= float(d_over)).sum())
        # samples with zero weights and a finite value whose right or lower neighbour texel (the taps a four-tap blend would read) is not
        zw = P.zero_weight_mask(c.w, c.h, c.bw, c.bh)
        x0, x1, _ = P.taps(c.w, c.bw)
        y0, y1, _ = P.taps(c.h, c.bh)
        other = ~np.isfinite(v64[y0][:, x1]) | ~np.isfinite(v64[y1][:, x0]) | ~np.isfinite(v64[y1][:, x1])
        here = np.isfinite(v64[y0][:, x0])
        counts["zero_weight_by_nonfinite"] += int((zw[..., None] & here & other).sum())
        counts["zero_weight_nan_neighbour"] += int((zw[..., None] & here & (np.isnan(v64[y0][:, x1]) | np.isnan(v64[y1][:, x0]))).sum())
    print("\npresent fuzz coverage:", counts)
    assert all(n > 0 for n in counts.values()), counts
    sizes = {((c.bw, c.bh), (c.w, c.h)) for c in cases}
    for want in (((7, 5), (32768, 1)), ((5, 7), (1, 32768)), ((1, 1), (13, 7)), ((9, 11), (1, 1)), ((63, 5), (63, 5)), ((64, 4), (64, 4)),
                 ((65, 3), (65, 3)), ((256, 256), (256, 256))):
        assert want in sizes, want
    assert {c.w for c in cases} >= {63, 64, 65} and any(c.half for c in cases) and any(not c.half for c in cases)
    # every f16 pattern in every channel, both layouts
    for c in cases[:2]:
        bits = c.bb.view(np.uint16)
        assert all(np.unique(bits[..., k]).size == 65536 for k in range(4)), c
    # the f32 NaN patterns travel as bits
    assert any(np.isin(np.array(PC.F32_NAN_BITS, np.uint32), c.bb.view(np.uint32)).all() for c in cases if not c.half)


def test_delta_is_four_times_the_measured_f32_error():
    """MEASURED_MAX is the largest |q32 - q| over the list.  One class of samples is left out of it and held separately: a colour whose
    tone-mapped value lies within 1e-6 (relative) of the sRGB threshold 0.0031308.  The two branches of linear_to_srgb differ there by 9.3e-4
    in q (10.3147 against 10.3157: the exponent is 0.41666, not 1 / 2.4), which is a step of the specification and not an error of f32; on
    which side of it an input within a few ulp lands is not decidable, and both sides round to the same byte, 10, far from a boundary."""
    worst, where, at_knee = 0.0, None, 0
    for c in PC.cases():
        q, q32 = _q(c), P.present_q32(c.bb, c.w, c.h)
        assert np.isfinite(q).all() and np.isfinite(q32).all(), c
        knee = np.zeros(q.shape, bool)
        with np.errstate(invalid="ignore"):
            knee[..., :3] = np.abs(P.aces(P.sample(c.bb, c.w, c.h)[..., :3]) / 0.0031308 - 1.0) <= 1e-6
        at_knee += int(knee.sum())
        assert (np.floor(q[knee] + 0.5) == 10).all() and (np.floor(q32[knee] + 0.5) == 10).all() and (np.abs(q32 - q)[knee] < 1e-3).all(), c
        e = float(np.abs(q32 - q)[~knee].max())
        if e > worst:
            worst, where = e, c
    lo, hi = 255 * 12.92 * 0.0031308, 255 * (1.055 * 0.0031308 ** 0.41666 - 0.055)
    assert 9e-4 < hi - lo < 1e-3 and np.floor(lo + 0.5 - PC.DELTA) == np.floor(hi + 0.5 + PC.DELTA) == 10
    print(f"\npresent fuzz: largest |q32 - q| over the list {worst:.3e} ({where}); MEASURED_MAX {PC.MEASURED_MAX:.3e}, DELTA {PC.DELTA:.3e}; "
          f"{at_knee} samples at the sRGB knee held apart")
    assert 0 < at_knee < 2000
    assert PC.DELTA == 4.0 * PC.MEASURED_MAX
    assert 0.5 * PC.MEASURED_MAX <= worst <= PC.MEASURED_MAX, worst


def test_undecided_bytes_are_few_and_the_boundary_case_has_none():
    und_total = n_total = 0
    for c in PC.cases():
        q = _q(c)
        und = P.undecided(q, PC.DELTA)
        und_total += int(und.sum())
        n_total += und.size
        if und.size >= 1000:
            assert und.mean() <= 0.005, (c, und.mean())
        if "boundaries" in c.tags:
            assert not und.any(), c
            z = q + 0.5
            assert (np.abs(z - np.round(z)) >= 2.0 * PC.DELTA).all()
            # ... and it does straddle: per channel the bytes 0 .. 255 all occur
            b = np.floor(z).astype(int)
            assert all(np.unique(b[..., k]).size == 256 for k in range(4)), c
    print(f"\npresent fuzz: {und_total} of {n_total} bytes undecided ({100.0 * und_total / n_total:.4f} %)")
    assert und_total <= 0.005 * n_total


def test_tone_map_is_monotone_over_the_non_negative_halves_and_ends_at_255(O):
    bits = np.arange(0x7C01, dtype=np.uint16)  # +0 .. +inf
    vals = np.concatenate([bits.view(np.float16), np.full(32768 - bits.size, np.inf, np.float16)]).astype(np.float32)
    bb = np.zeros((128, 256, 4), np.float32)  # powers of two: every sample has zero weights
    bb[..., 0] = bb[..., 1] = bb[..., 2] = vals.reshape(128, 256)
    for got in (O.present(bb, 256, 128), np.floor(P.present_q(bb, 256, 128) + 0.5).astype(np.uint8)):
        r = got[..., 0].reshape(-1).astype(int)
        assert (np.diff(r) >= 0).all() and r[0] == 0 and r[bits.size - 1] == 255 and r[-1] == 255
        assert (got[..., 1] == got[..., 0]).all() and (got[..., 2] == got[..., 0]).all()


def test_the_old_formula_fails_beyond_the_overflow_point():
    """The pass before its curve was extended by its limits, in three lines of f32: the rule rejects what it made of values beyond the overflow
    point (and accepts it below), so a kernel that still computes this turns the fuzz modules red."""
    n_over, d_over = PC.overflow_points()
    x = np.array([1.0, 65504.0, 1e10, np.nextafter(d_over, np.float32(0)), d_over, 1e30, np.inf, -np.inf, -1e30], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        old = x * (np.float32(2.51) * x + np.float32(0.03)) / (x * (np.float32(2.43) * x + np.float32(0.59)) + np.float32(0.14))
        c = np.where(np.isnan(old), np.float32(0), np.clip(old, np.float32(0), np.float32(1)))  # fmaxf(NaN, 0) = 0
        byte = np.floor(255.0 * P.srgb(c.astype(np.float64)) + 0.5)
    wrong, _ = P.judge(byte, P.tone_q(x), PC.DELTA)
    assert wrong.tolist() == [False, False, False, False, True, True, True, True, True], (byte, P.tone_q(x))
    assert (byte[wrong] == 0).all() and (P.tone_q(x)[wrong] > 255 - 1e-9).all()
