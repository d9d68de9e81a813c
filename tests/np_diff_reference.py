"""vk_steady_diffusion in numpy, written another way than tests/diff_restatement.c: no loop over voxels, but whole-array float32
operations on arrays padded by one voxel, one shifted view per neighbour, the six terms added in the rule's order; a colour is a mask.
numpy's float32 ufuncs round once per operation and fuse nothing, which is what the rule asks for.  It shares no code with the restatement;
the range predicate and the fill rule are the label reference's.  omega is taken as given."""
import numpy as np

import np_label_reference as NL

OFF = 0x7FC00000
F = np.float32


def quantise(t):
    """int64 of clamp(t) * 2^30, truncated; a NaN takes the lower clamp."""
    t = np.asarray(t, F)
    with np.errstate(invalid="ignore"):
        k = np.where(t >= F(-1048576.0), np.where(t <= F(1048576.0), t, F(1048576.0)), F(-1048576.0)).astype(F)
    return np.trunc((k * F(1073741824.0)).astype(np.float64)).astype(np.int64)


def converged(delta, fin, fout, delta_tol, flux_tol):
    return bool(float(F(delta)) <= float(F(delta_tol)) and abs(float(fin) - float(fout)) <= float(F(flux_tol)) * 0.5 * (float(fin) + float(fout)))


def apply(vol, kind, lo, hi, axis, spacing, omega, check_every, max_sweeps, delta_tol, flux_tol, gain, fill_out, box):
    """(c float32 [nz, ny, nx] with the bits OFF off the set, dense, result uint64 [12]: n_foreground, n_inlet, n_outlet, n_box, Fin_q,
    Fout_q, sum_c_q, sweeps, converged, the bits of delta, of omega and of the gain used)."""
    v = np.asarray(vol)
    nz, ny, nx = v.shape
    s = NL.foreground(v, kind, lo, hi, box)
    x0, y0, z0, x1, y1, z1 = box if box is not None else (0, 0, 0, nx, ny, nz)
    first, last = (x0, y0, z0)[axis], (x1, y1, z1)[axis] - 1
    coord = np.indices(v.shape)  # [z, y, x]
    along = coord[2 - axis]
    inlet, outlet = s & (along == first), s & (along == last)
    parity = (coord[0] + coord[1] + coord[2]) & 1
    w = [F(1.0 / float(int(spacing[k]) * int(spacing[k]))) for k in range(3)]
    g = F(2.0) * w[axis]
    omega = F(omega)
    sp = np.pad(s, 1)
    inner = (slice(1, -1),) * 3

    def view(a, k, side):  # the neighbour along axis k (0 x, 1 y, 2 z) on the given side, as an array of the unpadded shape
        sl = [slice(1, -1)] * 3
        sl[2 - k] = slice(0, -2) if side < 0 else slice(2, None)
        return a[tuple(sl)]

    # den does not change between sweeps: the same adds in the same order every time
    den = np.zeros(v.shape, F)
    for k in range(3):
        for side in (-1, 1):
            den = np.where(view(sp, k, side), den + w[k], den).astype(F)
    den = np.where(inlet, den + g, den).astype(F)
    den = np.where(outlet, den + g, den).astype(F)
    live = s & (den != 0)
    colours = [live & (parity == 0), live & (parity == 1)]
    c = np.full(v.shape, 0.5, F)
    cp = np.zeros((nz + 2, ny + 2, nx + 2), F)
    blocks, done, delta, fin, fout = 0, False, F(0.0), 0, 0
    safe_den = np.where(live, den, F(1.0)).astype(F)
    while blocks < max_sweeps // check_every and not done:
        for sweep in range(check_every):
            if sweep + 1 == check_every:
                delta = F(0.0)
            for m in colours:
                cp[inner] = c
                num = np.zeros(v.shape, F)
                for k in range(3):
                    for side in (-1, 1):
                        num = np.where(view(sp, k, side), num + w[k] * view(cp, k, side), num).astype(F)
                num = np.where(inlet, num + g, num).astype(F)
                gs = (num / safe_den).astype(F)
                nxt = (c + omega * (gs - c)).astype(F)
                if sweep + 1 == check_every and m.any():
                    delta = max(delta, np.abs((nxt - c).astype(F))[m].max())
                c = np.where(m, nxt, c).astype(F)
        blocks += 1
        fin = int(quantise(F(2.0) * (F(1.0) - c[inlet])).sum())
        fout = int(quantise(F(2.0) * c[outlet]).sum())
        done = converged(delta, fin, fout, delta_tol, flux_tol)
    k = F(gain) if F(gain) != 0 else F(1.0)
    dense = np.where(s, NL.fill_bits((c * k).astype(F), kind), np.full(v.shape, NL.fill_bits(fill_out, kind), v.dtype)).astype(v.dtype)
    u64 = lambda i: int(i) & 0xFFFFFFFFFFFFFFFF  # noqa: E731
    result = np.array([int(s.sum()), int(inlet.sum()), int(outlet.sum()), max(x1 - x0, 0) * max(y1 - y0, 0) * max(z1 - z0, 0), u64(fin), u64(fout), u64(quantise(c[s]).sum()),
                       blocks * check_every, int(done), int(F(delta).view(np.uint32)), int(omega.view(np.uint32)), int(k.view(np.uint32))], np.uint64)
    out = c.view(np.uint32).copy()
    out[~s] = OFF
    return out.view(F), dense, result
