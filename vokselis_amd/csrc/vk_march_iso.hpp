// vk_march_iso.hpp -- the loops of the cell march under first-hit isosurface rendering (vk_set_isosurface):
// march_mip() and march_mip_stream() of vk_march_mip.hpp with another operator on the filtered sample, one compare, x >= iso_k
// (vk_iso.hpp: iso_hit), and another exit: the hit sample's position stays in p.  The family's own: each loop's frame, condition, skip
// decision, operator and advance; the rest are the parts the MAX loops call (vk_march_parts.hpp; one loop for both: DESIGN.md section 13).
// Included by vk_march.hpp after vk_march_mip.hpp, and so part of every unit that includes vk_march.hpp;
// instantiated by raymarch_iso_kernel (vk_launch_iso.hip), its shadowing twin raymarch_iso_shadow_kernel (vk_launch_iso_shadow.hip) and the
// R16_UNORM units, through vk_march_kernel_body.hpp under ISO.  The refinement and the shade are the kernel body's epilogue, once per ray;
// iso_sample() below is what both fetch with, and iso_shadowed() at the end is the shadow ray of the shadowing kernels: these loops again.
#pragma once

namespace vk {

// march_mip() for the isosurface.  RayState::A carries X, the last sample's value; Gr, Gg, Gb are unused.  X is NaN at the start:
// x >= k is false for a NaN, so there is no hit yet whatever iso_k is (an R8 threshold far below the data overflows to iso_k = -inf,
// which a -inf would meet).  A ray ends when its iterations are used up or X >= iso_k.  The hit is folded into the loop condition, and the
// hitting iteration neither advances p nor uses up its iteration: p is the hit sample's own bits, the refinement starts from them, and
// `left` still counts that iteration, so the body knows a hit in the ray's first iteration by left being what it was.  The breaking
// iteration is counted (COUNT).  A cell whose distance byte is not 0 is empty under iso_cell_empty: no sample in it can hit, the walk
// skips it with the reference's own additions of p.  A resumed ray (BOUNDED) that has hit makes no further trip.
template <int VOL, bool SKIP, bool SAFE, bool COUNT, bool BOUNDED>
__device__ __forceinline__ bool march_iso(const VolumeDesc &V, RayState &r, const uint32_t budget, Census &cs, const uint32_t *lut,
                                          const float walk_cap, const float walk_cap_all, const float iso_k) {
    constexpr bool PACKED = is_cell_layout(VOL);
    float px = r.px, py = r.py, pz = r.pz, X = r.A;
    int nleft = -(int)r.left;  // minus the iterations left (as march())
    const float sx = r.sx, sy = r.sy, sz = r.sz;
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    const int mx = (int)V.nx - 1, my = (int)V.ny - 1, mz = (int)V.nz - 1;

    const SkipBound sb = skip_bound<SKIP>(sx, sy, sz, fnx, fny, fnz);  // per-ray constants of the skip bound
    const uint32_t doff = SKIP ? ((sx >= 0.0f ? 1u : 0u) | (sy >= 0.0f ? 2u : 0u) | (sz >= 0.0f ? 4u : 0u)) * V.dist_oct_stride : 0u;
    const uint32_t *luty = lut + (V.nx + 3), *lutz = lut + (V.nx + V.ny + 6);
    const __amdgpu_buffer_rsrc_t cells = cell_buffer(V.data, SAFE ? 0u : (uint32_t)V.max_off + (1u << V.sh_x));

    uint32_t trip = 0;
    while (nleft != 0 && !iso_hit(X, iso_k) && (!BOUNDED || trip < budget)) {
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
                // the skip decision of march_mip(), statement for statement; shared below it (as one function: DESIGN.md section 13)
                const float cap_now = __ballot(ca.d == 0) != 0ull ? walk_cap : walk_cap_all;
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
        X = lerp_yz(fy, fz, c00, c10, c01, c11);
        if (COUNT) { cs.n_iter++; cs.n_samp++; if (wave_leader()) cs.w_sample++; }
        if (!iso_hit(X, iso_k)) {  // the hit sample keeps its position and its iteration
            px = px + sx; py = py + sy; pz = pz + sz;
            nleft += 1;
        }
    }
    r.left = (uint32_t)(-nleft); r.px = px; r.py = py; r.pz = pz; r.A = X;
    return nleft != 0 && !iso_hit(X, iso_k);
}

// march_mip_stream() for the isosurface: the fast path without skipping, every trip samples, the next trip's cell requested before
// this trip's sample is evaluated.  The request needs the advanced position while the hit needs the sample's own, so the loop keeps
// two positions and uses them alternately, as it does its two cell buffers: neither a copy per trip nor a subtraction after the hit.
// The f32 operations on p and X are march_iso()'s, in the same order per variable.
template <int VOL, bool COUNT, bool CELL_LUT>
__device__ __forceinline__ bool march_iso_stream(const VolumeDesc &V, RayState &r, Census &cs, const uint32_t *lut, uint32_t budget, const float iso_k) {
    float ax = r.px, ay = r.py, az = r.pz, X = r.A;
    float bx = ax, by = ay, bz = az;
    uint32_t left = r.left;
    const float sx = r.sx, sy = r.sy, sz = r.sz;
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    const uint32_t *luty = lut + (V.nx + 3), *lutz = lut + (V.nx + V.ny + 6);
    const __amdgpu_buffer_rsrc_t cells = cell_buffer(V.data, (uint32_t)V.max_off + (1u << V.sh_x));
    if (!(left != 0u && !iso_hit(X, iso_k))) return false;
    const uint32_t lsh = CELL_LUT ? V.sh_x : 0u;
    float fx, fy, fz;
    CellBits<VOL> c0, c1;  // two cell buffers, used alternately
    {
        const float ux = fmaf(ax, fnx, -0.5f), uy = fmaf(ay, fny, -0.5f), uz = fmaf(az, fnz, -0.5f);
        fx = __builtin_amdgcn_fractf(ux); fy = __builtin_amdgcn_fractf(uy); fz = __builtin_amdgcn_fractf(uz);
        c0 = request_cell<VOL>(cells, lut, luty, lutz, lsh, ux, uy, uz);
    }
    // one trip: `cur` is the cell of position (cx, cy, cz); request `nxt` for the advanced position (nx, ny, nz) (request_cell: safe one
    // step past the ray's end too), evaluate `cur`; returns whether the ray goes on.  A hit leaves `left` as it is.
    auto trip = [&](const CellBits<VOL> &cur, CellBits<VOL> &nxt, const float cx, const float cy, const float cz, float &nx, float &ny, float &nz) -> bool {
        if (COUNT) { cs.n_look++; cs.n_iter++; cs.n_samp++; if (wave_leader()) { cs.w_outer++; cs.w_sample++; } }
        nx = cx + sx; ny = cy + sy; nz = cz + sz;
        const float ux = fmaf(nx, fnx, -0.5f), uy = fmaf(ny, fny, -0.5f), uz = fmaf(nz, fnz, -0.5f);
        nxt = request_cell<VOL>(cells, lut, luty, lutz, lsh, ux, uy, uz);
        float c00, c10, c01, c11;
        xlerp_cell<VOL>(cur, fx, c00, c10, c01, c11);
        X = lerp_yz(fy, fz, c00, c10, c01, c11);
        if (iso_hit(X, iso_k)) return false;
        left -= 1u;
        fx = __builtin_amdgcn_fractf(ux); fy = __builtin_amdgcn_fractf(uy); fz = __builtin_amdgcn_fractf(uz);
        return left != 0u;
    };
    bool alive = true, at_a = false;  // at_a: the ray's position on return is (ax, ay, az)
    for (;;) {
        if (!trip(c0, c1, ax, ay, az, bx, by, bz)) { alive = false; at_a = iso_hit(X, iso_k); break; }
        if (budget != 0xffffffffu && --budget == 0u) break;
        if (!trip(c1, c0, bx, by, bz, ax, ay, az)) { alive = false; at_a = !iso_hit(X, iso_k); break; }
        if (budget != 0xffffffffu && --budget == 0u) { at_a = true; break; }
    }
    asm volatile("" ::"v"(c0.v), "v"(c1.v));  // the last requests are consumed on the exit path too (march_stream())
    r.left = left; r.px = at_a ? ax : bx; r.py = at_a ? ay : by; r.pz = at_a ? az : bz; r.A = X;
    return alive;
}

// The sample at (qx, qy, qz) with what the shade needs of it (vk_light.hpp: lit_gradient's arguments), fetched through the family's
// own address path: the index tables in LDS on the fast path, the clamped 64-bit offset under SAFE, linear_taps on the LINEAR layouts.
// Never consults a skip map (cell_at without DIST).  The filter is the loops', bit for bit; y/z written out: lit_gradient takes l0, l1.
struct IsoSample {
    float x, dx00, dx10, dx01, dx11, c00, c10, c01, c11, l0, l1, fy, fz;
};
template <int VOL, bool SKIP, bool SAFE>
__device__ __forceinline__ IsoSample iso_sample(const VolumeDesc &V, const uint32_t *lut, const float qx, const float qy, const float qz) {
    constexpr bool PACKED = is_cell_layout(VOL);
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    const float ux = fmaf(qx, fnx, -0.5f), uy = fmaf(qy, fny, -0.5f), uz = fmaf(qz, fnz, -0.5f);
    int ix = cvt_floor_i32(ux), iy = cvt_floor_i32(uy), iz = cvt_floor_i32(uz);
    const float fx = __builtin_amdgcn_fractf(ux);
    IsoSample o;
    o.fy = __builtin_amdgcn_fractf(uy); o.fz = __builtin_amdgcn_fractf(uz);
    if constexpr (PACKED) {
        if constexpr (SAFE) { ix = med3_i32(ix, -1, (int)V.nx - 1); iy = med3_i32(iy, -1, (int)V.ny - 1); iz = med3_i32(iz, -1, (int)V.nz - 1); }
        // the loops' tables: cell indices in the skip kernels, byte offsets in the others (cell_kernel_lds)
        const CellAt ca = cell_at<SKIP, SAFE, false>(V, lut, lut + (V.nx + 3), lut + (V.nx + V.ny + 6), 0u, ix, iy, iz);
        xlerp_cell_dx<VOL>(load_cell<VOL, SAFE>(cell_buffer(V.data, (uint32_t)V.max_off + (1u << V.sh_x)), ca.cptr, ca.coff), fx, o.c00, o.c10, o.c01, o.c11, o.dx00, o.dx10, o.dx01, o.dx11);
    } else {
        float tp[8];
        linear_taps<VOL>(V, ix, iy, iz, tp);
        o.dx00 = tp[1] - tp[0]; o.dx10 = tp[3] - tp[2]; o.dx01 = tp[5] - tp[4]; o.dx11 = tp[7] - tp[6];
        xlerp_taps(tp, fx, o.c00, o.c10, o.c01, o.c11);
    }
    o.l0 = fmaf(o.fy, o.c10 - o.c00, o.c00); o.l1 = fmaf(o.fy, o.c11 - o.c01, o.c01);
    o.x = fmaf(o.fz, o.l1 - o.l0, o.l0);
    return o;
}

// The shadow ray of a surface point q (vk_set_shadows; vk_shadow.hpp): the loops above a second time, from q along
// the unit light direction Ld through the box [lo, hi] the primary ray marched, with the primary ray's step formula for Ld.  Returns
// whether a sample on it is at or above iso_k.  Called from the kernel body's epilogue by the wave's hit lanes together; Ld, lo, hi,
// dt_scale and bias are kernel arguments, so the step, the octant offset of the skip maps and the constants of the skip bound are
// wave-uniform and stay on the scalar unit.  Nothing is counted (COUNT = false, a Census of its own): the step image and the counters
// are the primary ray's.  The skip kernels walk with the loop and the distance maps, the fast path without skipping takes the
// pipelined loop, SAFE and LINEAR the plain one.  ts0 >= tb1 leaves no iteration: A stays NaN, no hit.
template <int VOL, bool SKIP, bool SAFE>
__device__ __forceinline__ bool iso_shadowed(const VolumeDesc &V, const uint32_t *lut, const float q[3], const float Ld[3], const float lo[3], const float hi[3],
                                             const float dt_scale, const float bias, const float walk_cap, const float walk_cap_all, const float iso_k) {
    constexpr bool USE_LUT = is_cell_layout(VOL) && !SAFE;
    float tb0, tb1;
    intersect_box(q, Ld, lo, hi, tb0, tb1);
    if (tb0 > tb1) return false;
    const float dtx = 1.0f / ((float)V.nx * fabsf(Ld[0]));
    const float dty = 1.0f / ((float)V.ny * fabsf(Ld[1]));
    const float dtz = 1.0f / ((float)V.nz * fabsf(Ld[2]));
    const float dts = dt_scale * fminf(dtx, fminf(dty, dtz));
    const float ts0 = shadow_ts0(tb0, bias, dts);
    RayState s;
    s.left = min(count_trips(ts0, tb1, dts), 0x7fffffffu);
    s.px = fmaf(ts0, Ld[0], q[0]); s.py = fmaf(ts0, Ld[1], q[1]); s.pz = fmaf(ts0, Ld[2], q[2]);
    s.sx = Ld[0] * dts; s.sy = Ld[1] * dts; s.sz = Ld[2] * dts;
    s.A = __builtin_nanf(""); s.Gr = 0.0f; s.Gg = 0.0f; s.Gb = 0.0f;
    s.out = 0u;
    Census cs;
    if constexpr (USE_LUT && !SKIP) march_iso_stream<VOL, false, false>(V, s, cs, lut, 0xffffffffu, iso_k);
    else if constexpr (SKIP) march_iso<VOL, true, SAFE, false, false>(V, s, 0xffffffffu, cs, USE_LUT ? lut : nullptr, walk_cap, walk_cap_all, iso_k);
    else march_iso<VOL, false, SAFE, false, false>(V, s, 0xffffffffu, cs, USE_LUT ? lut : nullptr, __builtin_inff(), __builtin_inff(), iso_k);
    return iso_hit(s.A, iso_k);
}

}  // namespace vk
