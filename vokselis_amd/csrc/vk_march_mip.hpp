// vk_march_mip.hpp -- the loops of the cell march under the maximum-intensity projection (vk_set_projection(VK_PROJ_MAX); DESIGN.md
// section 12): march() and march_stream() of vk_march.hpp with another operator on the filtered sample, U = mip_update(U, x) (vk_tf.hpp),
// the running maximum in table coordinates.  The family's own: each loop's frame, condition, skip decision, operator and advance.
// vk_march_parts.hpp's, and so the isosurface loops' too: the skip bound, cell_at, walk_exact, load_cell / request_cell, the taps and
// the lerps.  Included by vk_march.hpp, after the definitions it shares with that file's loops, and so part of every unit that
// includes vk_march.hpp; instantiated by raymarch_mip_kernel (vk_launch_mip.hip) alone, through vk_march_kernel_body.hpp under MIP.
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
    constexpr bool PACKED = is_cell_layout(VOL);
    float px = r.px, py = r.py, pz = r.pz, U = r.A;
    int nleft = -(int)r.left;  // minus the iterations left (as march())
    const float sx = r.sx, sy = r.sy, sz = r.sz;
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    const int mx = (int)V.nx - 1, my = (int)V.ny - 1, mz = (int)V.nz - 1;

    const SkipBound sb = skip_bound<SKIP>(sx, sy, sz, fnx, fny, fnz);  // per-ray constants of the skip bound
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
            const CellAt ca = cell_at<SKIP, SAFE>(V, lut, luty, lutz, doff, ix, iy, iz);
            if (SKIP && ca.d != 0) {
                if (BOUNDED) cs.skips++;
                // walks are capped in a trip in which other lanes sample (march(): the samplers pace the trip); any stop is exact
                const float cap_now = __ballot(ca.d == 0) != 0ull ? walk_cap : walk_cap_all;
                // samples j = 0 .. k - 1 are skipped, k = ceil(min r_i) clamped to [1, iterations left]: p += s, k times, the reference's additions
                const float rmin = fminf(sb.steps(fx, fy, fz, (float)ca.d), cap_now);
                const int kneg = walk_steps_neg(rmin, nleft);  // -k
                nleft -= kneg;
                if (COUNT) { cs.n_iter += (uint32_t)(-kneg); if (wave_leader()) cs.w_inner++; }
                walk_exact<COUNT>(px, py, pz, sx, sy, sz, kneg, cs);
                continue;
            }
            xlerp_cell<VOL>(load_cell<VOL, SAFE>(cells, ca.cptr, ca.coff), fx, c00, c10, c01, c11);
        } else {
            float tp[8];
            linear_taps<VOL>(V, ix, iy, iz, tp);
            xlerp_taps(tp, fx, c00, c10, c01, c11);
        }
        U = mip_update(U, lerp_yz(fy, fz, c00, c10, c01, c11), k1, k2, umax);
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
        c0 = request_cell<VOL>(cells, lut, luty, lutz, lsh, ux, uy, uz);
    }
    // one trip: request `nxt` for the advanced position (request_cell: safe one step past the ray's end too), evaluate `cur`; returns whether the ray goes on
    auto trip = [&](const CellBits<VOL> &cur, CellBits<VOL> &nxt) -> bool {
        if (COUNT) { cs.n_look++; cs.n_iter++; cs.n_samp++; if (wave_leader()) { cs.w_outer++; cs.w_sample++; } }
        px = px + sx; py = py + sy; pz = pz + sz;
        const float ux = fmaf(px, fnx, -0.5f), uy = fmaf(py, fny, -0.5f), uz = fmaf(pz, fnz, -0.5f);
        nxt = request_cell<VOL>(cells, lut, luty, lutz, lsh, ux, uy, uz);
        float c00, c10, c01, c11;
        xlerp_cell<VOL>(cur, fx, c00, c10, c01, c11);
        U = mip_update(U, lerp_yz(fy, fz, c00, c10, c01, c11), k1, k2, umax);
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
