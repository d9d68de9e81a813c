// vk_march_mip.hpp -- the loops of the cell march under the maximum-intensity projection (vk_set_projection(VK_PROJ_MAX); DESIGN.md
// section 12): march() and march_stream() of vk_march.hpp with another operator on the filtered sample, U = mip_update(U, x) (vk_tf.hpp),
// the running maximum in table coordinates.  Loops of their own: the compositing loops do not carry the operator.  Included by
// vk_march.hpp, after the definitions they share with its loops; called from vk_march_kernel_body.hpp under MIP.
#pragma once

namespace vk {

// march() of vk_march.hpp for the maximum projection.  RayState::A carries U (0 <= U <= umax, +0 at the start); Gr, Gg, Gb are unused.
// A ray ends when its iterations are used up or U has reached umax: no later sample can change the pixel (the counterpart of A >= 0.95;
// as there, the test is folded into the loop condition -- p is dead after the break, so advancing it first changes nothing observable,
// and the breaking iteration is counted).  A cell whose distance byte is not 0 is empty under mip_cell_empty: every sample in it
// leaves U bit for bit, so the walk skips it with the reference's own additions of p.  What the compositing loops do when no
// lane's alpha is non-zero has no counterpart here: every sample is one fma, one compare-select and one min.
template <int VOL, bool SKIP, bool SAFE, bool COUNT, bool BOUNDED>
__device__ __forceinline__ bool march_mip(const VolumeDesc &V, RayState &r, const uint32_t budget, Census &cs, const uint32_t *lut,
                                          const float walk_cap, const float walk_cap_all, const float k1, const float k2, const float umax) {
    constexpr bool PACKED = (VOL == VOL_P8 || VOL == VOL_P16 || VOL == VOL_PF16);
    float px = r.px, py = r.py, pz = r.pz, U = r.A;
    int nleft = -(int)r.left;  // minus the iterations left (as march())
    const float sx = r.sx, sy = r.sy, sz = r.sz;
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    const int mx = (int)V.nx - 1, my = (int)V.ny - 1, mz = (int)V.nz - 1;

    // per-ray constants of the skip bound: march()'s, with its margins
    float idux = 0.f, iduy = 0.f, iduz = 0.f, skax = 0.f, skay = 0.f, skaz = 0.f, skbx = 0.f, skby = 0.f, skbz = 0.f;
    if (SKIP) {
        const float dux = fabsf(sx) * fnx, duy = fabsf(sy) * fny, duz = fabsf(sz) * fnz;  // cells per step
        idux = __builtin_amdgcn_rcpf(dux); iduy = __builtin_amdgcn_rcpf(duy); iduz = __builtin_amdgcn_rcpf(duz);
        const float n_walk = (float)(kDistRadius + 1) * __builtin_amdgcn_rcpf(fmaxf(dux, fmaxf(duy, duz)));
        const float mg = fmaf(n_walk * 0x1p-24f, fmaxf(fnx, fmaxf(fny, fnz)), 0.01f);
        constexpr float sc = 1.0f - 0x1p-12f, cst = -0.01f;
        skax = (sx >= 0.0f ? -idux : idux) * sc; skay = (sy >= 0.0f ? -iduy : iduy) * sc; skaz = (sz >= 0.0f ? -iduz : iduz) * sc;
        skbx = fmaf((sx >= 0.0f ? -mg : -1.0f - mg) * idux, sc, cst);
        skby = fmaf((sy >= 0.0f ? -mg : -1.0f - mg) * iduy, sc, cst);
        skbz = fmaf((sz >= 0.0f ? -mg : -1.0f - mg) * iduz, sc, cst);
        idux *= sc; iduy *= sc; iduz *= sc;
    }
    const uint32_t doff = SKIP ? ((sx >= 0.0f ? 1u : 0u) | (sy >= 0.0f ? 2u : 0u) | (sz >= 0.0f ? 4u : 0u)) * V.dist_oct_stride : 0u;
    const uint32_t *luty = lut + (V.nx + 3), *lutz = lut + (V.nx + V.ny + 6);
    const __amdgpu_buffer_rsrc_t cells = cell_buffer(V.data, SAFE ? 0u : (uint32_t)V.max_off + (1u << V.sh_x));

    uint32_t trip = 0;
    while (nleft != 0 && U < umax && (!BOUNDED || trip < budget)) {
        if (BOUNDED) ++trip;
        if (COUNT) { cs.n_look++; if (wave_leader()) cs.w_outer++; }
        const float ux = fmaf(px, fnx, -0.5f), uy = fmaf(py, fny, -0.5f), uz = fmaf(pz, fnz, -0.5f);
        int ix = cvt_floor_i32(ux), iy = cvt_floor_i32(uy), iz = cvt_floor_i32(uz);
        const float fx = __builtin_amdgcn_fractf(ux), fy = __builtin_amdgcn_fractf(uy), fz = __builtin_amdgcn_fractf(uz);
        float c00, c10, c01, c11;  // x-lerped corners
        if (PACKED) {
            if (SAFE) { ix = med3_i32(ix, -1, mx); iy = med3_i32(iy, -1, my); iz = med3_i32(iz, -1, mz); }
            const int bx = ix >> 2, by = iy >> 2, bz = iz >> 2;
            const char *cptr = nullptr;
            uint32_t d = 0, coff = 0;
            if (SAFE) {
                int64_t off = (int64_t)bz * (int64_t)V.kz + (int64_t)(by * (int)V.ky + bx * (int)V.kx) +
                              (int64_t)((iz << V.sh_z) + (iy << V.sh_y) + (ix << V.sh_x)) + (int64_t)V.c0;
                off = off < 0 ? 0 : (off > (int64_t)V.max_off ? (int64_t)V.max_off : off);
                cptr = reinterpret_cast<const char *>(V.data) + off;
                if (SKIP) d = V.dist[(uint64_t)(off >> V.sh_x) + doff];
            } else {
                // cell index (SKIP) / cell byte offset (!SKIP) from the per-axis tables in LDS; entry i + 2 is voxel i
                const uint32_t idx = lut[ix + 2] + luty[iy + 2] + lutz[iz + 2];
                coff = SKIP ? (uint32_t)(idx << V.sh_x) : idx;
                if (SKIP) d = V.dist[idx + doff];
            }
            if (SKIP && d != 0) {
                if (BOUNDED) cs.skips++;
                // walks are capped in a trip in which other lanes sample (march(): the samplers pace the trip); any stop is exact
                const float cap_now = __ballot(d == 0) != 0ull ? walk_cap : walk_cap_all;
                const float fd = (float)d;
                const float rx = fmaf(fx, skax, fmaf(fd, idux, skbx));
                const float ry = fmaf(fy, skay, fmaf(fd, iduy, skby));
                const float rz = fmaf(fz, skaz, fmaf(fd, iduz, skbz));
                // samples j = 0 .. k - 1 are skipped, k = ceil(min r_i) clamped to [1, iterations left]: p += s, k times, the reference's additions
                const float rmin = fminf(fminf(fminf(rx, ry), rz), cap_now);
                const int kneg = walk_steps_neg(rmin, nleft);  // -k
                nleft -= kneg;
                if (COUNT) { cs.n_iter += (uint32_t)(-kneg); if (wave_leader()) cs.w_inner++; }
                px = px + sx; py = py + sy; pz = pz + sz;
                uint32_t m = (uint32_t)(-1 - kneg);  // the steps after the first
                for (uint32_t q = m >> 2; q != 0u; --q) {
#pragma unroll
                    for (int j = 0; j < 4; j++) { px = px + sx; py = py + sy; pz = pz + sz; }
                    if (COUNT) { if (wave_leader()) cs.w_inner++; }
                }
                for (m &= 3u; m != 0u; --m) { px = px + sx; py = py + sy; pz = pz + sz; }
                continue;
            }
            CellBits<VOL> cb;
            if (SAFE) {
                if constexpr (VOL == VOL_P8) { const uint2 c = *reinterpret_cast<const uint2 *>(cptr); cb.v.x = c.x; cb.v.y = c.y; }
                else { const uint4 c = *reinterpret_cast<const uint4 *>(cptr); cb.v.x = c.x; cb.v.y = c.y; cb.v.z = c.z; cb.v.w = c.w; }
            } else {
                cb = load_cell<VOL>(cells, coff);
            }
            xlerp_cell<VOL>(cb, fx, c00, c10, c01, c11);
        } else {
            const int x0 = clampi(ix, 0, mx), x1 = clampi(ix + (ix < 0x7fffffff), 0, mx);
            const int y0 = clampi(iy, 0, my), y1 = clampi(iy + (iy < 0x7fffffff), 0, my);
            const int z0 = clampi(iz, 0, mz), z1 = clampi(iz + (iz < 0x7fffffff), 0, mz);
            const size_t sy_ = V.nx, sz_ = (size_t)V.nx * V.ny;
            const size_t r00 = y0 * sy_ + z0 * sz_, r10 = y1 * sy_ + z0 * sz_;
            const size_t r01 = y0 * sy_ + z1 * sz_, r11 = y1 * sy_ + z1 * sz_;
            float tp[8];
            if (VOL == VOL_LINEAR_U8) {
                const uint8_t *v = reinterpret_cast<const uint8_t *>(V.data);
                tp[0] = (float)v[r00 + x0]; tp[1] = (float)v[r00 + x1]; tp[2] = (float)v[r10 + x0]; tp[3] = (float)v[r10 + x1];
                tp[4] = (float)v[r01 + x0]; tp[5] = (float)v[r01 + x1]; tp[6] = (float)v[r11 + x0]; tp[7] = (float)v[r11 + x1];
            } else {
                const uint16_t *v = reinterpret_cast<const uint16_t *>(V.data);
                tp[0] = h2f(v[r00 + x0]); tp[1] = h2f(v[r00 + x1]); tp[2] = h2f(v[r10 + x0]); tp[3] = h2f(v[r10 + x1]);
                tp[4] = h2f(v[r01 + x0]); tp[5] = h2f(v[r01 + x1]); tp[6] = h2f(v[r11 + x0]); tp[7] = h2f(v[r11 + x1]);
            }
            c00 = fmaf(fx, tp[1] - tp[0], tp[0]); c10 = fmaf(fx, tp[3] - tp[2], tp[2]);
            c01 = fmaf(fx, tp[5] - tp[4], tp[4]); c11 = fmaf(fx, tp[7] - tp[6], tp[6]);
        }
        const float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
        const float x = fmaf(fz, c1 - c0, c0);
        U = mip_update(U, x, k1, k2, umax);
        if (COUNT) { cs.n_iter++; cs.n_samp++; if (wave_leader()) cs.w_sample++; }
        px = px + sx; py = py + sy; pz = pz + sz;
        nleft += 1;
    }
    r.left = (uint32_t)(-nleft); r.px = px; r.py = py; r.pz = pz; r.A = U;
    return nleft != 0 && U < umax;
}

// march_stream() of vk_march.hpp for the maximum projection: the fast path without skipping, every trip samples, the next trip's cell
// requested before this trip's sample is evaluated.  The f32 operations on p and U are march_mip()'s, in the same order per variable.
template <int VOL, bool COUNT, bool CELL_LUT>
__device__ __forceinline__ bool march_mip_stream(const VolumeDesc &V, RayState &r, Census &cs, const uint32_t *lut, uint32_t budget,
                                                 const float k1, const float k2, const float umax) {
    float px = r.px, py = r.py, pz = r.pz, U = r.A;
    uint32_t left = r.left;
    const float sx = r.sx, sy = r.sy, sz = r.sz;
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    const uint32_t *luty = lut + (V.nx + 3), *lutz = lut + (V.nx + V.ny + 6);
    const __amdgpu_buffer_rsrc_t cells = cell_buffer(V.data, (uint32_t)V.max_off + (1u << V.sh_x));
    if (!(left != 0u && U < umax)) return false;
    const uint32_t lsh = CELL_LUT ? V.sh_x : 0u;
    float fx, fy, fz;
    CellBits<VOL> c0, c1;  // two cell buffers, used alternately
    {
        const float ux = fmaf(px, fnx, -0.5f), uy = fmaf(py, fny, -0.5f), uz = fmaf(pz, fnz, -0.5f);
        fx = __builtin_amdgcn_fractf(ux); fy = __builtin_amdgcn_fractf(uy); fz = __builtin_amdgcn_fractf(uz);
        c0 = load_cell<VOL>(cells, (lut[cvt_floor_i32(ux) + 2] + luty[cvt_floor_i32(uy) + 2] + lutz[cvt_floor_i32(uz) + 2]) << lsh);
    }
    // one trip: request `nxt` for the advanced position (a clamped table entry, a bounds-checked buffer load: inside the cell array
    // also one step past the ray's end), evaluate `cur`; returns whether the ray goes on
    auto trip = [&](const CellBits<VOL> &cur, CellBits<VOL> &nxt) -> bool {
        if (COUNT) { cs.n_look++; cs.n_iter++; cs.n_samp++; if (wave_leader()) { cs.w_outer++; cs.w_sample++; } }
        px = px + sx; py = py + sy; pz = pz + sz;
        const float ux = fmaf(px, fnx, -0.5f), uy = fmaf(py, fny, -0.5f), uz = fmaf(pz, fnz, -0.5f);
        nxt = load_cell<VOL>(cells, (lut[cvt_floor_i32(ux) + 2] + luty[cvt_floor_i32(uy) + 2] + lutz[cvt_floor_i32(uz) + 2]) << lsh);
        float c00, c10, c01, c11;
        xlerp_cell<VOL>(cur, fx, c00, c10, c01, c11);
        const float l0 = fmaf(fy, c10 - c00, c00), l1 = fmaf(fy, c11 - c01, c01);
        U = mip_update(U, fmaf(fz, l1 - l0, l0), k1, k2, umax);
        left -= 1u;
        fx = __builtin_amdgcn_fractf(ux); fy = __builtin_amdgcn_fractf(uy); fz = __builtin_amdgcn_fractf(uz);
        return left != 0u && U < umax;
    };
    bool alive = true;
    for (;;) {
        if (!trip(c0, c1)) { alive = false; break; }
        if (budget != 0xffffffffu && --budget == 0u) break;
        if (!trip(c1, c0)) { alive = false; break; }
        if (budget != 0xffffffffu && --budget == 0u) break;
    }
    asm volatile("" ::"v"(c0.v), "v"(c1.v));  // the last requests are consumed on the exit path too (march_stream())
    r.left = left; r.px = px; r.py = py; r.pz = pz; r.A = U;
    return alive;
}

}  // namespace vk
