// vk_march_parts.hpp -- the statement groups the march loops are built from, each written once: the loops' counters, the built-in
// palette and the compositing, the per-ray constants of the skip bound (with the proof of its margins), the cell address, fetch,
// pipelined request and x-lerp of the PACKED layouts, the exact skip walk, the y/z lerp, the eight taps of the LINEAR layouts, and the
// fetch and decode of the dense 9^3-brick and quad layouts.  Included by vk_march.hpp, and through it by the loops of vk_march_mip.hpp,
// vk_march_iso.hpp and vk_staged.hpp.  Plain inlined functions that keep the statement order of the sites they replaced: the loops'
// register allocation follows how their source is factored (who uses what, and the sites that kept their own
// text), and tools/isa_diff.py holds every change here to the parent's device code.
#pragma once

#include "vk_common.hpp"
#include "vk_texel.hpp"  // CellBits, load_cell through a pointer

namespace vk {

// ---- what the loops count -----------------------------------------------------------------------------------------------------
struct Census {  // SIMT execution census + step counters (COUNT builds only)
    uint32_t n_iter = 0, n_samp = 0, w_outer = 0, w_inner = 0, w_sample = 0, n_look = 0, n_fb = 0;
    uint32_t skips = 0;  // trips that skipped (every build: drives the adaptive probing policy)
    // the built-in skip kernels (COUNT builds): wave-level sample executions in which every sampling lane's alpha came out 0 (the upper bound on what
    // the lone-speckle codes can take away), and lane-steps those codes proved transparent without a sample
    uint32_t w_zero = 0, n_proven = 0;
    // per-trip log of the wave (COUNT builds, debug bit 6; docs/archive/tools/repack_census.py): entry = live lanes | samplers << 7 | samplers whose alpha is
    // not 0 << 14 | wave-level walk iterations << 21
    uint32_t *log = nullptr;
    uint32_t log_cap = 0, trip_no = 0;
};

// ---- the built-in palette and the compositing (raycast_naive.wgsl:70-81, :108-114) -------------------------------------------
// vertigo(): 0.5 + 0.5*cos(6.28318*(c*a + d)).  v_cos_f32 takes its argument in revolutions, so the phase is a single fma with
// constants pre-divided by 2*pi.  The loops accumulate G = sum w*cos(phase) and add the 0.5s once per ray: C = 0.5 A + 0.5 G.
__device__ __forceinline__ void palette_cos(float a, float &cr, float &cg, float &cb) {
    constexpr double kk = 6.28318 / 6.283185307179586476925;
    constexpr float pc0 = (float)(1.0 * kk), pc1 = (float)(1.7 * kk), pc2 = (float)(0.4 * kk);
    constexpr float pd1 = (float)(0.15 * kk), pd2 = (float)(0.20 * kk);
    cr = __builtin_amdgcn_cosf(a * pc0);
    cg = __builtin_amdgcn_cosf(fmaf(a, pc1, pd1));
    cb = __builtin_amdgcn_cosf(fmaf(a, pc2, pd2));
}
// :112-114, front to back: the sample's colour (the palette's cosines or the table's rgb) under its alpha
__device__ __forceinline__ void composite(float a, float cr, float cg, float cb, float &A, float &Gr, float &Gg, float &Gb) {
    const float w = (1.0f - A) * a;
    Gr = fmaf(w, cr, Gr); Gg = fmaf(w, cg, Gg); Gb = fmaf(w, cb, Gb);
    A = A + w;
}
__device__ __forceinline__ void palette_composite(float a, float &A, float &Gr, float &Gg, float &Gb) {
    float cr, cg, cb;
    palette_cos(a, cr, cg, cb);
    composite(a, cr, cg, cb, A, Gr, Gg, Gb);
}

// ---- the skip bound -----------------------------------------------------------------------------------------------------------
// A cell's distance byte d says: every cell within Chebyshev distance d - 1 of this one is empty.  Sample j of a ray sits at
// u + j*du (cells); it is skipped iff its cell provably stays in that range on every axis: j*|du| < d - f (moving up) or
// j*|du| <= f + d - 1 (moving down), minus the margins: j < r = min_i r_i.
// Per axis r_i = room_i / |du_i| with room_i = d - f_i (moving up) or f_i + d - 1 (moving down), minus a 0.02-cell margin that
// covers the rounding of the accumulated position (<= 1e-3 cells); folded into two fmas: r_i = f_i * ska_i + (d * idu_i + skb_i).
struct SkipBound {
    float idux, iduy, iduz, skax, skay, skaz, skbx, skby, skbz;
    // r for the sample at lerp weights f in a cell of distance byte d (as a float)
    __device__ __forceinline__ float steps(float fx, float fy, float fz, float fd) const {
        const float rx = fmaf(fx, skax, fmaf(fd, idux, skbx));
        const float ry = fmaf(fy, skay, fmaf(fd, iduy, skby));
        const float rz = fmaf(fz, skaz, fmaf(fd, iduz, skbz));
        return fminf(fminf(rx, ry), rz);
    }
};
// the per-ray constants (all 0 without SKIP: never read)
template <bool SKIP>
__device__ __forceinline__ SkipBound skip_bound(float sx, float sy, float sz, float fnx, float fny, float fnz) {
    float idux = 0.f, iduy = 0.f, iduz = 0.f, skax = 0.f, skay = 0.f, skaz = 0.f, skbx = 0.f, skby = 0.f, skbz = 0.f;
    if (SKIP) {
        // rcp (1 ulp) is enough: these constants only bound a skip length, with the margins below.
        const float dux = fabsf(sx) * fnx, duy = fabsf(sy) * fny, duz = fabsf(sz) * fnz;  // cells per step
        idux = __builtin_amdgcn_rcpf(dux); iduy = __builtin_amdgcn_rcpf(duy); iduz = __builtin_amdgcn_rcpf(duz);
        // Position margin, in cells: a walk crosses at most kDistRadius + 1 cells of its fastest axis,
        // i.e. n <= 25 / max(du) steps, each adding <= 2^-25 of rounding to a coordinate in [0, 1]
        // (x n_i cells); doubled, plus 0.01 for the rounding of u itself.
        const float n_walk = (float)(kDistRadius + 1) * __builtin_amdgcn_rcpf(fmaxf(dux, fmaxf(duy, duz)));
        const float mg = fmaf(n_walk * 0x1p-24f, fmaxf(fnx, fmaxf(fny, fnz)), 0.01f);
        // (the walk counts its steps: no margin for a drifting loop variable; 2^-12 covers rcp and the fmas, 0.01 of a step on top)
        constexpr float sc = 1.0f - 0x1p-12f, cst = -0.01f;
        skax = (sx >= 0.0f ? -idux : idux) * sc; skay = (sy >= 0.0f ? -iduy : iduy) * sc; skaz = (sz >= 0.0f ? -iduz : iduz) * sc;
        skbx = fmaf((sx >= 0.0f ? -mg : -1.0f - mg) * idux, sc, cst);
        skby = fmaf((sy >= 0.0f ? -mg : -1.0f - mg) * iduy, sc, cst);
        skbz = fmaf((sz >= 0.0f ? -mg : -1.0f - mg) * iduz, sc, cst);
        idux *= sc; iduy *= sc; iduz *= sc;
    }
    return {idux, iduy, iduz, skax, skay, skaz, skbx, skby, skbz};
}

// ---- the cells of the PACKED layouts ------------------------------------------------------------------------------------------
// PIN: mark the load volatile (aux bit 31: compiler-only, nothing changes in the encoding) so that it
// is issued where it is written -- a prefetch must not be sunk behind the loop's exit branch.
template <int VOL, bool PIN = false>
__device__ __forceinline__ CellBits<VOL> load_cell(__amdgpu_buffer_rsrc_t rs, uint32_t off) {
    constexpr int aux = PIN ? (int)0x80000000u : 0;
    CellBits<VOL> c;
    if constexpr (VOL == VOL_P8) c.v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, aux);
    else c.v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, aux);
    return c;
}

// SAFE (no index tables): the byte offset of voxel (ix, iy, iz)'s cell, the 64-bit closed form of the tables' sum, clamped into
// the cell array whatever the indices are; the cell at that offset comes through a plain pointer (vk_texel.hpp: load_cell, and cell_offset,
// this function's twin on uint32_t indices in 64-bit arithmetic).  The arithmetic is vk_hostmath.hpp's cell_offset_clamped, which
// tests/fastpath_fuzz.cpp runs under UBSan on every shape the upload accepts (by * ky is a 64-bit product: it passes 2^31 on flat
// volumes of 4 GiB and more).
__device__ __forceinline__ int64_t safe_cell_offset(const VolumeDesc &V, int ix, int iy, int iz) {
    return cell_offset_clamped(V.kz, V.c0, V.max_off, V.kx, V.ky, V.sh_x, V.sh_y, V.sh_z, ix, iy, iz);
}

// Where voxel (ix, iy, iz)'s cell is, and under DIST its distance byte in the ray's map (`doff`: the octant's offset).  SAFE: the clamped
// offset as a pointer; otherwise the sum of the per-axis tables in LDS, entry i + 2 is voxel i -- a cell index in the skip kernels'
// tables (SKIP), a cell byte offset in the others' -- as a byte offset.  (DIST = false: iso_sample, through either kind of table.)
struct CellAt { const char *cptr = nullptr; uint32_t coff = 0, d = 0; };
template <bool SKIP, bool SAFE, bool DIST = SKIP>
__device__ __forceinline__ CellAt cell_at(const VolumeDesc &V, const uint32_t *lut, const uint32_t *luty, const uint32_t *lutz, uint32_t doff, int ix, int iy, int iz) {
    CellAt c;
    if (SAFE) {
        const int64_t off = safe_cell_offset(V, ix, iy, iz);
        c.cptr = reinterpret_cast<const char *>(V.data) + off;
        if (DIST) c.d = V.dist[(uint64_t)(off >> V.sh_x) + doff];
    } else {
        const uint32_t idx = lut[ix + 2] + luty[iy + 2] + lutz[iz + 2];
        c.coff = SKIP ? (uint32_t)(idx << V.sh_x) : idx;
        if (DIST) c.d = V.dist[idx + doff];
    }
    return c;
}
// ... and the cell there: through the pointer under SAFE, else the bounds-checked buffer load
template <int VOL, bool SAFE>
__device__ __forceinline__ CellBits<VOL> load_cell(__amdgpu_buffer_rsrc_t cells, const char *cptr, uint32_t coff) {
    if constexpr (SAFE) return load_cell<VOL>(cptr);
    else return load_cell<VOL>(cells, coff);
}

// The pipelined loops' request: the cell at cell coordinates (ux, uy, uz) through the tables (`lsh`: V.sh_x where they hold cell indices,
// 0 where byte offsets).  A clamped table entry and a bounds-checked buffer load: inside the cell array also one step past the ray's end.
template <int VOL>
__device__ __forceinline__ CellBits<VOL> request_cell(__amdgpu_buffer_rsrc_t cells, const uint32_t *lut, const uint32_t *luty, const uint32_t *lutz,
                                                      uint32_t lsh, float ux, float uy, float uz) {
    return load_cell<VOL>(cells, (lut[cvt_floor_i32(ux) + 2] + luty[cvt_floor_i32(uy) + 2] + lutz[cvt_floor_i32(uz) + 2]) << lsh);
}

// The exact walk over k = -kneg >= 1 skipped samples: p += s, k times, the reference's own additions -- the first, then four per loop
// iteration (counted by the wave leader under COUNT), then the remainder.  (`cs` whole: a reference to the one counter moved 12 COUNT kernels to class C.)
template <bool COUNT>
__device__ __forceinline__ void walk_exact(float &px, float &py, float &pz, float sx, float sy, float sz, int kneg, Census &cs) {
    px = px + sx; py = py + sy; pz = pz + sz;
    uint32_t m = (uint32_t)(-1 - kneg);  // the steps after the first
    for (uint32_t q = m >> 2; q != 0u; --q) {
#pragma unroll
        for (int j = 0; j < 4; j++) { px = px + sx; py = py + sy; pz = pz + sz; }
        if (COUNT) { if (wave_leader()) cs.w_inner++; }
    }
    for (m &= 3u; m != 0u; --m) { px = px + sx; py = py + sy; pz = pz + sz; }
}

// the y and z lerps of the four x-lerped corners: the filtered sample
__device__ __forceinline__ float lerp_yz(float fy, float fz, float c00, float c10, float c01, float c11) {
    const float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
    return fmaf(fz, c1 - c0, c0);
}

// x-lerps of one cell: c00, c10, c01, c11 (the four x edges of the footprint), and the four x-differences t1 - t0, t3 - t2,
// t5 - t4, t7 - t6 they are made with (the lit kernels' gradient, vk_light.hpp); PACKED_PAIRS returns its stored deltas, which are
// those differences exactly for u8 data
template <int VOL>
__device__ __forceinline__ void xlerp_cell_dx(const CellBits<VOL> &cb, float fx, float &c00, float &c10, float &c01, float &c11,
                                              float &dx00, float &dx10, float &dx01, float &dx11) {
    if constexpr (VOL == VOL_P8) {
        const uint32_t lo = cb.v.x, hi = cb.v.y;
        float t0_ = (float)(lo & 0xffu), t1_ = (float)((lo >> 8) & 0xffu), t2_ = (float)((lo >> 16) & 0xffu), t3_ = (float)(lo >> 24);
        float t4_ = (float)(hi & 0xffu), t5_ = (float)((hi >> 8) & 0xffu), t6_ = (float)((hi >> 16) & 0xffu), t7_ = (float)(hi >> 24);
        dx00 = t1_ - t0_; dx10 = t3_ - t2_; dx01 = t5_ - t4_; dx11 = t7_ - t6_;
        c00 = fmaf(fx, dx00, t0_); c10 = fmaf(fx, dx10, t2_);
        c01 = fmaf(fx, dx01, t4_); c11 = fmaf(fx, dx11, t6_);
    } else {
        union { u32x4_t u; half2_t h[4]; } c;
        c.u = cb.v;
        if constexpr (VOL == VOL_PU16) {
            // u16 taps, two per word: one conversion each (v_cvt_f32_u32 with a word select), exact; the differences are exact too (integers below 2^16)
            const uint32_t w0 = cb.v.x, w1 = cb.v.y, w2 = cb.v.z, w3 = cb.v.w;
            float a0 = (float)(w0 & 0xffffu), a1 = (float)(w0 >> 16), a2 = (float)(w1 & 0xffffu), a3 = (float)(w1 >> 16);
            float a4 = (float)(w2 & 0xffffu), a5 = (float)(w2 >> 16), a6 = (float)(w3 & 0xffffu), a7 = (float)(w3 >> 16);
            dx00 = a1 - a0; c00 = fmaf(fx, dx00, a0); dx10 = a3 - a2; c10 = fmaf(fx, dx10, a2);
            dx01 = a5 - a4; c01 = fmaf(fx, dx01, a4); dx11 = a7 - a6; c11 = fmaf(fx, dx11, a6);
        } else if constexpr (VOL == VOL_P16) {
            // (tap, delta) pairs: delta = t1 - t0 is exact in f16 for u8 data -> v_fma_mix_f32
            dx00 = (float)c.h[0].y; dx10 = (float)c.h[1].y; dx01 = (float)c.h[2].y; dx11 = (float)c.h[3].y;
            c00 = fmaf(fx, dx00, (float)c.h[0].x); c10 = fmaf(fx, dx10, (float)c.h[1].x);
            c01 = fmaf(fx, dx01, (float)c.h[2].x); c11 = fmaf(fx, dx11, (float)c.h[3].x);
        } else {
            float a0 = (float)c.h[0].x, a1 = (float)c.h[0].y, a2 = (float)c.h[1].x, a3 = (float)c.h[1].y;
            float a4 = (float)c.h[2].x, a5 = (float)c.h[2].y, a6 = (float)c.h[3].x, a7 = (float)c.h[3].y;
            // (difference, lerp, difference, lerp: the order the kernels without lighting were scheduled from)
            dx00 = a1 - a0; c00 = fmaf(fx, dx00, a0); dx10 = a3 - a2; c10 = fmaf(fx, dx10, a2);
            dx01 = a5 - a4; c01 = fmaf(fx, dx01, a4); dx11 = a7 - a6; c11 = fmaf(fx, dx11, a6);
        }
    }
}
template <int VOL>
__device__ __forceinline__ void xlerp_cell(const CellBits<VOL> &cb, float fx, float &c00, float &c10, float &c01, float &c11) {
    float dx00, dx10, dx01, dx11;
    xlerp_cell_dx<VOL>(cb, fx, c00, c10, c01, c11, dx00, dx10, dx01, dx11);
}
// the x-lerps of eight taps, tap index dx + 2*dy + 4*dz (the layouts that fetch taps, not cells)
__device__ __forceinline__ void xlerp_taps(const float tp[8], float fx, float &c00, float &c10, float &c01, float &c11) {
    c00 = fmaf(fx, tp[1] - tp[0], tp[0]); c10 = fmaf(fx, tp[3] - tp[2], tp[2]);
    c01 = fmaf(fx, tp[5] - tp[4], tp[4]); c11 = fmaf(fx, tp[7] - tp[6], tp[6]);
}

// ---- the eight taps of the LINEAR layouts (clamped indices: always inside the array) -------------------------------------------
template <int VOL>
__device__ __forceinline__ void linear_taps(const VolumeDesc &V, int ix, int iy, int iz, float tp[8]) {
    const int mx = (int)V.nx - 1, my = (int)V.ny - 1, mz = (int)V.nz - 1;
    int x0 = clampi(ix, 0, mx), x1 = clampi(ix + (ix < 0x7fffffff), 0, mx);
    int y0 = clampi(iy, 0, my), y1 = clampi(iy + (iy < 0x7fffffff), 0, my);
    int z0 = clampi(iz, 0, mz), z1 = clampi(iz + (iz < 0x7fffffff), 0, mz);
    size_t sy_ = V.nx, sz_ = (size_t)V.nx * V.ny;
    size_t r00 = y0 * sy_ + z0 * sz_, r10 = y1 * sy_ + z0 * sz_;
    size_t r01 = y0 * sy_ + z1 * sz_, r11 = y1 * sy_ + z1 * sz_;
    if (VOL == VOL_LINEAR_U8) {
        const uint8_t *v = reinterpret_cast<const uint8_t *>(V.data);
        tp[0] = (float)v[r00 + x0]; tp[1] = (float)v[r00 + x1]; tp[2] = (float)v[r10 + x0]; tp[3] = (float)v[r10 + x1];
        tp[4] = (float)v[r01 + x0]; tp[5] = (float)v[r01 + x1]; tp[6] = (float)v[r11 + x0]; tp[7] = (float)v[r11 + x1];
    } else if (VOL == VOL_LINEAR_U16) {
        const uint16_t *v = reinterpret_cast<const uint16_t *>(V.data);
        tp[0] = (float)v[r00 + x0]; tp[1] = (float)v[r00 + x1]; tp[2] = (float)v[r10 + x0]; tp[3] = (float)v[r10 + x1];
        tp[4] = (float)v[r01 + x0]; tp[5] = (float)v[r01 + x1]; tp[6] = (float)v[r11 + x0]; tp[7] = (float)v[r11 + x1];
    } else {
        const uint16_t *v = reinterpret_cast<const uint16_t *>(V.data);
        tp[0] = h2f(v[r00 + x0]); tp[1] = h2f(v[r00 + x1]); tp[2] = h2f(v[r10 + x0]); tp[3] = h2f(v[r10 + x1]);
        tp[4] = h2f(v[r01 + x0]); tp[5] = h2f(v[r01 + x1]); tp[6] = h2f(v[r11 + x0]); tp[7] = h2f(v[r11 + x1]);
    }
}

// ---- the dense layouts: the fetched words of one sample, then its eight taps ---------------------------------------------------
// Both address a sample by its cell coords c = i + 1 in [0, n] (indices clamped: always inside the array): brick c >> 3, local c & 7.
struct DenseWords { uint32_t a, b, c, d; };
constexpr bool is_b9(int VOL) { return VOL == VOL_B9U8 || VOL == VOL_B9F16; }
constexpr bool is_quads(int VOL) { return VOL == VOL_Q8 || VOL == VOL_QF16; }

// 9^3 bricks: the taps sit at local (l, l+1) per axis, offsets {0,1} + {0,9} + {0,81} from one base; the words are the x pairs at
// (y, z) = (0,0) (1,0) (0,1) (1,1)
template <int VOL>
__device__ __forceinline__ DenseWords b9_request(const VolumeDesc &V, int ix, int iy, int iz) {
    const int cx = med3_i32(ix, -1, (int)V.nx - 1) + 1, cy = med3_i32(iy, -1, (int)V.ny - 1) + 1, cz = med3_i32(iz, -1, (int)V.nz - 1) + 1;
    const uint32_t brick = (uint32_t)(((cz >> 3) * (int)V.nby + (cy >> 3)) * (int)V.nbx + (cx >> 3));
    const uint32_t local = (uint32_t)((cz & 7) * 81 + (cy & 7) * 9 + (cx & 7));
    typedef uint16_t u16_unaligned __attribute__((aligned(1)));
    typedef uint32_t u32_unaligned __attribute__((aligned(2)));
    DenseWords q;
    if (VOL == VOL_B9U8) {
        const uint8_t *b = reinterpret_cast<const uint8_t *>(V.data) + ((uint64_t)brick * 729u + local);
        q.a = *reinterpret_cast<const u16_unaligned *>(b); q.b = *reinterpret_cast<const u16_unaligned *>(b + 9);
        q.c = *reinterpret_cast<const u16_unaligned *>(b + 81); q.d = *reinterpret_cast<const u16_unaligned *>(b + 90);
    } else {
        const uint16_t *b = reinterpret_cast<const uint16_t *>(V.data) + ((uint64_t)brick * 729u + local);
        q.a = *reinterpret_cast<const u32_unaligned *>(b); q.b = *reinterpret_cast<const u32_unaligned *>(b + 9);
        q.c = *reinterpret_cast<const u32_unaligned *>(b + 81); q.d = *reinterpret_cast<const u32_unaligned *>(b + 90);
    }
    return q;
}
template <int VOL>
__device__ __forceinline__ void b9_decode(const DenseWords &q, float tp[8]) {
    if (VOL == VOL_B9U8) {
        tp[0] = (float)(q.a & 0xffu); tp[1] = (float)(q.a >> 8); tp[2] = (float)(q.b & 0xffu); tp[3] = (float)(q.b >> 8);
        tp[4] = (float)(q.c & 0xffu); tp[5] = (float)(q.c >> 8); tp[6] = (float)(q.d & 0xffu); tp[7] = (float)(q.d >> 8);
    } else {
        tp[0] = h2f(q.a & 0xffffu); tp[1] = h2f(q.a >> 16); tp[2] = h2f(q.b & 0xffffu); tp[3] = h2f(q.b >> 16);
        tp[4] = h2f(q.c & 0xffffu); tp[5] = h2f(q.c >> 16); tp[6] = h2f(q.d & 0xffffu); tp[7] = h2f(q.d >> 16);
    }
}
// quads: one load per sample, two consecutive elements.  u8: a = element(x), b = element(x+1), a byte per (y, z) corner;
// f16: (a, b) = element(x), (c, d) = element(x+1)
template <int VOL>
__device__ __forceinline__ DenseWords quad_request(const VolumeDesc &V, int ix, int iy, int iz) {
    const int cx = med3_i32(ix, -1, (int)V.nx - 1) + 1, cy = med3_i32(iy, -1, (int)V.ny - 1) + 1, cz = med3_i32(iz, -1, (int)V.nz - 1) + 1;
    const uint32_t brick = (uint32_t)(((cz >> 3) * (int)V.nby + (cy >> 3)) * (int)V.nbx + (cx >> 3));
    const uint32_t local = (uint32_t)(((cz & 7) * 8 + (cy & 7)) * 9 + (cx & 7));
    const uint64_t e = (uint64_t)brick * 576u + local;
    typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));  // elements are 4 / 8 bytes: the pair is under-aligned
    typedef uint32_t u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
    DenseWords q;
    if (VOL == VOL_Q8) {
        const u32x2_a4 v = *reinterpret_cast<const u32x2_a4 *>(reinterpret_cast<const uint32_t *>(V.data) + e);
        q.a = v.x; q.b = v.y; q.c = 0; q.d = 0;
    } else {
        const u32x4_a8 v = *reinterpret_cast<const u32x4_a8 *>(reinterpret_cast<const uint2 *>(V.data) + e);
        q.a = v.x; q.b = v.y; q.c = v.z; q.d = v.w;
    }
    return q;
}
template <int VOL>
__device__ __forceinline__ void quad_decode(const DenseWords &q, float tp[8]) {
    if (VOL == VOL_Q8) {
        tp[0] = (float)(q.a & 0xffu); tp[2] = (float)((q.a >> 8) & 0xffu); tp[4] = (float)((q.a >> 16) & 0xffu); tp[6] = (float)(q.a >> 24);
        tp[1] = (float)(q.b & 0xffu); tp[3] = (float)((q.b >> 8) & 0xffu); tp[5] = (float)((q.b >> 16) & 0xffu); tp[7] = (float)(q.b >> 24);
    } else {
        tp[0] = h2f(q.a & 0xffffu); tp[2] = h2f(q.a >> 16); tp[4] = h2f(q.b & 0xffffu); tp[6] = h2f(q.b >> 16);
        tp[1] = h2f(q.c & 0xffffu); tp[3] = h2f(q.c >> 16); tp[5] = h2f(q.d & 0xffffu); tp[7] = h2f(q.d >> 16);
    }
}

}  // namespace vk
