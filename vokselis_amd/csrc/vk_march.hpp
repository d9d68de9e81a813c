// vk_march.hpp -- NAIVE_TRILINEAR (raycast_naive.wgsl:83-125) on the cell layouts (and the LINEAR / 9^3 / quad comparison layouts).
// The loops march / march_stream / march_dense_stream, RayState, and raymarch_naive_kernel around the shared kernel body
// (vk_march_kernel_body.hpp).  Included by vk_launch_cells.hip for that kernel, by vk_launch_tf.hip and vk_launch_lit.hip, whose
// kernels instantiate the same loops with TF / LIT, by vk_launch_mip.hip and vk_launch_iso.hip for the loops of vk_march_mip.hpp and
// vk_march_iso.hpp (included below), and by vk_staged.hpp (vk_launch_staged.hip) for RayState, Census, clear_inactive_strip and the
// palette.  The statement groups the loops share, and Census, which they count into, are vk_march_parts.hpp's.
#pragma once

#include "vk_common.hpp"
#include "vk_exactdiv.hpp"
#include "vk_march_parts.hpp"
#include "vk_iso.hpp"
#include "vk_light.hpp"
#include "vk_shadow.hpp"
#include "vk_tf.hpp"
#include "vk_trips.hpp"

namespace vk {

// ... and copied into LDS by every wave of the march: a handful of 16-byte loads instead of ~200 VALU
// instructions of index arithmetic per wave.
__device__ __forceinline__ void load_cell_luts(const VolumeDesc &V, uint32_t *lut, uint32_t lane) {
    const uint32_t n4 = cell_lut_entries(V.nx, V.ny, V.nz) >> 2;
    const uint4 *src = reinterpret_cast<const uint4 *>(V.lut);
    uint4 *dst = reinterpret_cast<uint4 *>(lut);
    for (uint32_t e = lane; e < n4; e += 64u) dst[e] = src[e];
}

// -k for a walk of k = ceil(r) steps, 1 <= k <= iterations left (nleft = -left < 0): floor(-r) in one conversion (it saturates), clamped in one v_med3
__device__ __forceinline__ int walk_steps_neg(float r, int nleft) {
    int k;
    asm("v_cvt_flr_i32_f32_e64 %0, -%1\n\tv_med3_i32 %0, %0, %2, -1" : "=&v"(k) : "v"(r), "v"(nleft));
    return k;
}

// The runtime transfer function (vk_tf.hpp): entries i and i + 1 of the table, lerped per channel.  The index is clamped to
// [0, n - 2] whatever x is (a NaN reads entry 0): the two 16-byte loads stay inside the table.
__device__ __forceinline__ void tf_lookup(const TfDesc &D, float x, float &cr, float &cg, float &cb, float &ca) {
    const float u = tf_u(x, D.k1, D.k2, D.umax);
    const int i = tf_index(u, D.imax);
    const float f = u - (float)i;
    const float4 *T = reinterpret_cast<const float4 *>(D.rgba);
    const float4 t0 = T[i], t1 = T[i + 1];
    cr = fmaf(f, t1.x - t0.x, t0.x); cg = fmaf(f, t1.y - t0.y, t0.y);
    cb = fmaf(f, t1.z - t0.z, t0.z); ca = fmaf(f, t1.w - t0.w, t0.w);
}

// ---- the march, resumable ---------------------------------------------------------------------
// Everything a ray needs to continue: the accumulators of the reference loop (p, alpha, colour sums), its per-ray constants and
// where its pixel goes.  64 bytes.
// The loop variable of raycast_naive.wgsl:101 is not among them.  t feeds nothing but its own test `t < t1`, so the march carries
// `left`, the number of iterations the loop has still to make -- count_trips() (vk_trips.hpp) computes the loop's trip count from
// (t0, t1, dt) exactly, rounding by rounding, once per ray (round 5).
struct RayState {
    uint32_t left;       // iterations of :101 not made yet
    float px, py, pz, sx, sy, sz, A, Gr, Gg, Gb;
    uint32_t out;        // pixel index into the launch's output
    uint32_t pad[4];
};
static_assert(sizeof(RayState) == 64, "RayState is one 64-byte record");

// Runs at most `budget` trips of the reference loop (raycast_naive.wgsl:101-119) on the state and
// returns whether the ray is still alive.  State in, state out: a ray marched in several pieces
// goes through exactly the same f32 operations as one marched in one go.
//
// SAFE=false (the fast path of the PACKED layouts) looks the cell index up instead of computing it:
// idx = Tx[ix] + Ty[iy] + Tz[iz] with three small per-axis tables in LDS (`lut`, filled by the kernel:
// see load_cell_luts).  Three ds_read_b32 (not VALU) + one v_add3 replace the 14 integer VALU
// instructions of the closed form -- the loop is VALU-issue bound.  Every table entry is a valid
// non-negative partial index, so any combination of entries stays inside the cell array: no clamp.
// The tables hold voxels [-2, n] and NOTHING here keeps an index inside them: an index beyond reads
// the next axis' table, the padding or whatever follows in LDS, and the skip kernels read the distance
// byte with a plain global load at that sum.  What keeps the indices inside is the host's rule for
// launching this build at all -- cell_march_fast (vk_hostmath.hpp) bounds the camera distance AND the
// length of the ray, because the f32 loop drifts by half an ulp of t and of p per trip and a long ray
// keeps stepping after it has left the box -- and tests/fastpath_fuzz.cpp holds that rule to a replay of
// the loop.  The guarantee is needed for, and audited for, that plain load of the distance byte: every
// sampled position at any dt_scale, and the probe-ahead position for dt_scale <= 1.25.  The pipelined
// loops without a skip map (march_stream and its iso / MAX twins) request the cell one step past the
// ray's end at ANY dt_scale, up to dt_scale cells past the box: above 1.5 cells that index is outside
// the tables, and harmless only because an LDS read outside the allocation returns 0, the cell comes
// through a bounds-checked buffer load, and the value is never used.
//
// WALK: how a run of k exactly transparent steps advances the reference's position (p += s, k times: raycast_naive.wgsl:118; the loop
// variable of :101 is the integer `left`, see RayState: left -= k).
//   WALK_LOOP  the additions themselves, four steps per loop iteration, capped per trip: bit-exact, the default.
//   WALK_FMA   VK_RENDER_FAST_WALK, tolerance mode: one real addition, then k - 1 more steps as ONE fma with the rounded increment of
//              that addition, v_1 + m (v_1 - v_0).  Inside a binade every rounded addition of the same addend moves an accumulator
//              by the same amount, so this IS the reference's value unless the coordinate crosses a power of two during the walk;
//              there it parts from the reference by at most (steps after the crossing) x half an ulp (positions agree to ~2e-4 cell).
//              The number of iterations is the reference's whatever the walk does (`left` is exact), unless the alpha >= 0.95
//              early-out flips (profiles/r04_walk_modes.txt).  No cap: a walk of any length costs the same dozen instructions.
//   (Cutting the closed form at every binade boundary makes it exact again -- and 15 - 37 % slower than the loop: every crossing
//   costs the lane another probing trip.  docs/archive/experiments/skip_walk_binade_cut_closed_form.patch)
enum WalkKind : int { WALK_LOOP = 0, WALK_FMA = 2 };

//
// AHEAD (LF_PROBE_AHEAD; the fast path of the skip kernels): a trip needs two fetches one after the other -- the cell's distance byte, then, if it is 0,
// the cell -- and a heavy wave's chain of sampling trips pays both latencies per step.  With AHEAD the distance byte of the NEXT position is requested
// while this trip's sample is evaluated: a lane that samples advances p and t (the reference's additions, :118 -- neither depends on the sample)
// right after requesting its cell, locates the next position and requests its distance, then filters and composites.  One byte load is wasted
// when the ray ends with that sample.  Walkers locate their new position at the end of their walk, as they did at the top of the next trip before.
// Per ray the same operations in the same order on every variable.
//
// TF (the table kernels of vk_launch_tf.hip): the runtime transfer function replaces transfer_alpha and the palette (tf_lookup).
// DECODES: false for the bounded loop compiled into the probe-ahead kernel (its launches never take it): that kernel keeps no corner table
// (kSpeckleLutBytes) and reads a lone-speckle code as a cell to sample wherever it meets one.
// LIT (vk_launch_lit.hip; needs TF): the table colour is shaded by the sample's gradient (vk_light.hpp: lit_gradient, lit_shade) before it is
// composited; alpha, and with it every trip, walk and exit, is the table's.
template <int VOL, bool SKIP, bool SAFE, bool COUNT, bool BOUNDED = false, int WALK = WALK_LOOP, bool AHEAD = false, bool TF = false, bool LIT = false, bool DECODES = true>
__device__ __forceinline__ bool march(const VolumeDesc &V, RayState &r, const uint32_t budget, Census &cs,
                                      const uint32_t *lut = nullptr, const float walk_cap = __builtin_inff(), const float walk_cap_all = __builtin_inff(),
                                      const TfDesc *tfd = nullptr, const LightDesc *ld = nullptr, const LitRay *lr = nullptr) {
    static_assert(!LIT || TF, "lighting shades the table's colour");
    constexpr bool PACKED = is_cell_layout(VOL);
    constexpr bool BRICK9 = (VOL == VOL_B9U8 || VOL == VOL_B9F16);
    static_assert(!AHEAD || (PACKED && SKIP && !SAFE && !BOUNDED), "probe-ahead: the skip kernels' fast path, unbounded");
    constexpr bool CODED = SKIP && !TF && (VOL == VOL_P8 || VOL == VOL_P16);  // the maps this instantiation reads carry lone-speckle codes (see the trip)
    // ... and it decodes them.  The probe-ahead trip does not: its lone waves pay for every instruction of a trip, and a sample costs them one fetch as a
    // proven step would.  There a coded cell is what it was, a cell to sample: the byte read as a signed one makes that the same two compares as
    // before (at its use: a conversion where the byte is requested would wait for it there, and undo the probe-ahead).
    constexpr bool DECODE = CODED && !AHEAD && DECODES;
    float px = r.px, py = r.py, pz = r.pz, A = r.A, Gr = r.Gr, Gg = r.Gg, Gb = r.Gb;
    int nleft = -(int)r.left;  // minus the iterations left (counts up to 0: a walk's -k = floor(-r) comes out of one conversion)
    const float sx = r.sx, sy = r.sy, sz = r.sz;
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    uint32_t &n_iter = cs.n_iter, &n_samp = cs.n_samp, &w_outer = cs.w_outer, &w_inner = cs.w_inner, &w_sample = cs.w_sample, &n_look = cs.n_look;
    const int mx = (int)V.nx - 1, my = (int)V.ny - 1, mz = (int)V.nz - 1;

    const SkipBound sb = skip_bound<SKIP>(sx, sy, sz, fnx, fny, fnz);  // per-ray constants of the skip bound
    // this ray's octant selects its distance map (bit i: moving up on axis i, as in ska/skb above)
    const uint32_t doff = SKIP ? ((sx >= 0.0f ? 1u : 0u) | (sy >= 0.0f ? 2u : 0u) | (sz >= 0.0f ? 4u : 0u)) * V.dist_oct_stride : 0u;
    const uint32_t *luty = lut + (V.nx + 3), *lutz = lut + (V.nx + V.ny + 6);
    const __amdgpu_buffer_rsrc_t cells = cell_buffer(V.data, SAFE ? 0u : (uint32_t)V.max_off + (1u << V.sh_x));

    // One exit test per trip: `t < t1` (:101, here: iterations left) and the alpha early-out (:115-117) are folded into the
    // loop condition; p is dead after the break, so advancing it unconditionally (:118) changes nothing observable.
    uint32_t trip = 0;  // wave-uniform: the active lanes of a wave entered the loop together
    // AHEAD: where the ray stands, carried from trip to trip: lerp weights, cell index, and the cell's distance byte (possibly still in flight)
    float a_fx = 0.0f, a_fy = 0.0f, a_fz = 0.0f;
    uint32_t a_idx = 0, a_d = 0;
    // a cell's distance byte; where lone-speckle codes are decoded sign-extended (the load does it), so that a code (>= 128) is a negative word: the
    // one compare a trip among plain cells pays for them
    auto dist_at = [&](uint64_t i) -> uint32_t { return DECODE ? (uint32_t)(int32_t)(int8_t)V.dist[i] : (uint32_t)V.dist[i]; };
    auto locate = [&](float qx, float qy, float qz) {
        const float ux = fmaf(qx, fnx, -0.5f), uy = fmaf(qy, fny, -0.5f), uz = fmaf(qz, fnz, -0.5f);
        a_fx = __builtin_amdgcn_fractf(ux); a_fy = __builtin_amdgcn_fractf(uy); a_fz = __builtin_amdgcn_fractf(uz);
        a_idx = lut[cvt_floor_i32(ux) + 2] + luty[cvt_floor_i32(uy) + 2] + lutz[cvt_floor_i32(uz) + 2];
        // A request made for a ray that turns out to have ended looks one step past the ray's last sample: <= dt_scale cells further on any axis.
        // The tables carry one clamped entry beyond i = -1 and i = n - 1, which covers 1.5 cells past the box; the host sets LF_PROBE_AHEAD only for
        // dt_scale <= 1.25 (vk_render.hip), which leaves 0.25 cells for how far the f32 loop itself has carried the last sample out of the box --
        // set-up rounding plus half an ulp of t and of p per trip.  The host launches this build only where that stays below 0.25 cells
        // (vk_hostmath.hpp: cell_march_fast, which counts the trips of the longest ray), so the index is a table entry and the map is read inside
        // its allocation.  (No branch around the request, and a plain global load: an exec-masked region, or a bounds-checked buffer load, gives
        // most of the gain back.)
        a_d = dist_at(a_idx + doff);
    };
    if (AHEAD) locate(px, py, pz);
    while (nleft != 0 && A < 0.95f && (!BOUNDED || trip < budget)) {
        if (BOUNDED) ++trip;
        if (COUNT) { n_look++; if (wave_leader()) w_outer++; }
        uint32_t *le = nullptr;
        if (COUNT && cs.log) {
            if (cs.trip_no < cs.log_cap) { le = cs.log + cs.trip_no; atomicAdd(le, 1u); }
            cs.trip_no++;
        }
        const float ux = AHEAD ? 0.0f : fmaf(px, fnx, -0.5f), uy = AHEAD ? 0.0f : fmaf(py, fny, -0.5f), uz = AHEAD ? 0.0f : fmaf(pz, fnz, -0.5f);
        int ix = AHEAD ? 0 : cvt_floor_i32(ux), iy = AHEAD ? 0 : cvt_floor_i32(uy), iz = AHEAD ? 0 : cvt_floor_i32(uz);
        float fx = AHEAD ? a_fx : __builtin_amdgcn_fractf(ux), fy = AHEAD ? a_fy : __builtin_amdgcn_fractf(uy), fz = AHEAD ? a_fz : __builtin_amdgcn_fractf(uz);
        float c00, c10, c01, c11;  // x-lerped corners
        float dx00 = 0.0f, dx10 = 0.0f, dx01 = 0.0f, dx11 = 0.0f;  // LIT: the x-differences of the taps
        if (PACKED) {
            if (SAFE) { ix = med3_i32(ix, -1, mx); iy = med3_i32(iy, -1, my); iz = med3_i32(iz, -1, mz); }
            const char *cptr = nullptr;
            uint32_t d = 0, coff = 0;
            // (cell_at's block in this loop's own text, with dist_at and AHEAD: through cell_at 16 COUNT kernels changed -- DESIGN.md section 13)
            if (SAFE) {
                const int64_t off = safe_cell_offset(V, ix, iy, iz);
                cptr = reinterpret_cast<const char *>(V.data) + off;
                if (SKIP) d = dist_at((uint64_t)(off >> V.sh_x) + doff);
            } else if (AHEAD) {
                coff = (uint32_t)(a_idx << V.sh_x);
                d = a_d;
            } else {
                // cell index (SKIP) / cell byte offset (!SKIP) from the per-axis tables; entry i + 2 is voxel i
                const uint32_t idx = lut[ix + 2] + luty[iy + 2] + lutz[iz + 2];
                coff = SKIP ? (uint32_t)(idx << V.sh_x) : idx;
                if (SKIP) d = dist_at(idx + doff);
            }
            // Lone-speckle cells (built-in transfer, u8 cells; vk_tf.hpp: speckle_code, speckle_proven, with the proof): a distance byte >= 128 is no
            // distance.  The cell is not empty -- one tap is above the threshold -- but the byte says how much weight the hot corner may get before a
            // sample's alpha can leave +0.  A lane proven below it walks exactly this one step (the word 256: non-zero, so a walker, and its low byte,
            // which is all the walk's length reads, is 0: no room on any axis, k = 1; the next position is probed afresh, in the same cell or not).
            // A lane not proven samples the cell, as every lane in such a cell did before.  A wave among plain cells pays one compare and the branch
            // over the region.  Before `samplers`: a trip whose only non-empty cells were proven transparent walks under walk_cap_all.
            if constexpr (DECODE) {
                if ((int32_t)d < 0) {
                    asm volatile("" : "+v"(d));  // (keeps this an exec-masked region, skipped by the wave when no lane is in it: if-converted, every trip pays the decode)
                    if constexpr (SAFE) d = speckle_proven(d, fx, fy, fz) ? 256u : 0u;
                    else {  // the corner's o_i from the table behind the index tables (vk_common.hpp: kSpeckleLutBytes): one LDS read for the bit work
                        const float4 o = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(lut + cell_lut_entries(V.nx, V.ny, V.nz)) + (d & 0x70u));
                        d = speckle_below(d, o.z, o.x, o.y, fx, fy, fz) ? 256u : 0u;  // (stored y, z, x: the pair the packed subtraction takes comes first)
                    }
                }
            }
            // A trip in which some lanes sample is paced by them: whatever a walker covers beyond a few steps it covers while
            // the samplers -- and every walker with a shorter walk -- wait for the longest walk of the wave (the walk loop ran
            // 3.9 iterations of four steps per trip with 19 of 64 lanes active).  In such a trip walks are capped; the walker
            // probes again next trip, which the wave makes anyway.  Any stop is exact: what is not skipped now is probed again.
            // (One compare serves the branch and the wave-level test; the cap is a scalar.)
            // (one compare serves the branch and the wave-level test; the cap is chosen on the scalar unit, as bits)
            const bool walker = SKIP && (DECODE ? (int32_t)d > 0 : (CODED ? (int8_t)d > 0 : d != 0));  // (a code left undecoded is negative: a cell to sample)
            const unsigned long long samplers = SKIP ? __ballot(!walker) : 0ull;
            uint32_t cap_now;  // (s_cmp + s_cselect: written as a ternary the compiler builds two branches and five moves around it; C2 batches -0.6 %)
            asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, %2, %3" : "=s"(cap_now) : "s"(samplers), "s"(__builtin_amdgcn_readfirstlane(__float_as_uint(walk_cap))), "s"(__builtin_amdgcn_readfirstlane(__float_as_uint(walk_cap_all))) : "scc");
            if (walker) {
                if (BOUNDED) cs.skips++;  // (a proven speckle step votes with the skips: it was not sampled)
                // Samples j = 0 .. k - 1 are skipped, k = ceil(r) (j < r keeps a sample inside the empty range; the current sample, j = 0,
                // sits in an empty cell: k >= 1), at most the trip's cap and at most the iterations the loop has left -- every skipped
                // iteration is one the reference makes (it passes `t < t1` on the reference's own t: that is what `left` counts).
                // The walk advances the reference's position, p += s, k times: the same f32 additions in the same order.
                float rmin = sb.steps(fx, fy, fz, CODED ? (float)(d & 0xffu) : (float)d);  // (v_cvt_f32_ubyte0 either way)
                if (COUNT && CODED && d == 256u) { n_samp++; cs.n_proven++; }  // a step in a non-empty cell, as before: S_sampled keeps its meaning
                if constexpr (WALK == WALK_FMA) {
                    // one real addition, the other k - 1 as one fma with that addition's rounded increment (tolerance: see WalkKind)
                    const float x_1 = px + sx, y_1 = py + sy, z_1 = pz + sz;
                    const int kneg = walk_steps_neg(rmin, nleft);  // -k
                    const float m = (float)(-1 - kneg);
                    const float dx_q = x_1 - px, dy_q = y_1 - py, dz_q = z_1 - pz;
                    px = fmaf(m, dx_q, x_1); py = fmaf(m, dy_q, y_1); pz = fmaf(m, dz_q, z_1);
                    nleft -= kneg;
                    if (COUNT) { n_iter += (uint32_t)(-kneg); if (wave_leader()) { w_inner++; if (le) atomicAdd(le, 1u << 21); } }
                    if (AHEAD) locate(px, py, pz);
                    continue;
                }
                asm("v_min_f32 %0, %1, %2" : "=v"(rmin) : "s"(cap_now), "v"(rmin));  // (a known-quiet scalar: no canonicalise)
                // m = k - 1: the steps after the first.  Single-frame launches (AHEAD) round it down to even -- the odd step is left to the next
                // trip's probe (any stop is exact) and the walk loses a branch: the lone chains of a single frame pay per instruction
                // (C2 single frame -3.7 %; batches +2 %: they keep the odd step)
                const uint32_t m = ~(uint32_t)walk_steps_neg(rmin, nleft) & (AHEAD ? ~1u : ~0u);
                const int c = (int)~m;  // -k
                nleft -= c;
                if (COUNT) { n_iter += (uint32_t)(-c); if (wave_leader()) { w_inner++; if (le) atomicAdd(le, 1u << 21); } }
                px = px + sx; py = py + sy; pz = pz + sz;
                // four skipped iterations per trip of the walk (the counter's decrement is its own test: v_sub_co)
                for (uint32_t q = m >> 2; !__builtin_usub_overflow(q, 1u, &q);) {
#pragma unroll
                    for (int j = 0; j < 4; j++) { px = px + sx; py = py + sy; pz = pz + sz; }
                    if (COUNT) { if (wave_leader()) { w_inner++; if (le) atomicAdd(le, 1u << 21); } }
                }
                if (!AHEAD && (m & 1u)) {
                    asm volatile("" : "+v"(px));
                    px = px + sx; py = py + sy; pz = pz + sz;
                }
                if (m & 2u) {
                    // (the empty asm keeps this an exec-masked region: if-converted, the two steps are computed for every lane and
                    // then selected by v_cndmask through VCC in a row, ~16 issue cycles each -- profiles/r03_ubench_valu_issue_rate.txt --
                    // twice the cost of a whole four-step walk iteration)
                    asm volatile("" : "+v"(px));
                    px = px + sx; py = py + sy; pz = pz + sz;
                    px = px + sx; py = py + sy; pz = pz + sz;
                }
                if (AHEAD) locate(px, py, pz);
                continue;
            }
            const CellBits<VOL> cb = load_cell<VOL, SAFE>(cells, cptr, coff);
            if (AHEAD) {
                // :118 and :101's increment (one iteration fewer left) now -- neither depends on the sample -- then the next position's distance byte is requested
                // under this sample's arithmetic (fx, fy, fz keep THIS position's weights)
                px = px + sx; py = py + sy; pz = pz + sz;
                nleft += 1;
                locate(px, py, pz);
            }
            if constexpr (LIT) xlerp_cell_dx<VOL>(cb, fx, c00, c10, c01, c11, dx00, dx10, dx01, dx11);
            else xlerp_cell<VOL>(cb, fx, c00, c10, c01, c11);
        } else if (BRICK9) {
            float tp[8];
            b9_decode<VOL>(b9_request<VOL>(V, ix, iy, iz), tp);
            xlerp_taps(tp, fx, c00, c10, c01, c11);
        } else {
            float tp[8];
            linear_taps<VOL>(V, ix, iy, iz, tp);
            if constexpr (LIT) { dx00 = tp[1] - tp[0]; dx10 = tp[3] - tp[2]; dx01 = tp[5] - tp[4]; dx11 = tp[7] - tp[6]; }
            xlerp_taps(tp, fx, c00, c10, c01, c11);
        }
        float c0 = fmaf(fy, c10 - c00, c00), c1 = fmaf(fy, c11 - c01, c01);
        float r = fmaf(fz, c1 - c0, c0);
        float a, tr = 0.0f, tg = 0.0f, tb = 0.0f;
        if constexpr (TF) tf_lookup(*tfd, r, tr, tg, tb, a);
        else a = transfer_alpha<transfer_scale(VOL)>(r);
        if (COUNT && le) atomicAdd(le, (1u << 7) + (a != 0.0f ? 1u << 14 : 0u));
        if (SKIP) {
            // A cell is non-empty as soon as one of its 8 taps is above the threshold; the FILTERED value of a sample inside it
            // often is not (a lone voxel just above it, a silhouette), and then alpha is exactly 0: w = 0, every accumulator
            // takes +0 (the cosines are finite).  When that holds for every lane sampling in this trip -- it mostly does in
            // the executions that serve one or two lanes -- the palette and the compositing are left out: 17 of the 45
            // instructions, no bit changes.
            if (__ballot(a != 0.0f) == 0ull) {
                if (COUNT) { n_iter++; n_samp++; if (wave_leader()) { w_sample++; if constexpr (!TF) cs.w_zero++; } }
                if (!AHEAD) {
                    px = px + sx; py = py + sy; pz = pz + sz;  // :118
                    nleft += 1;
                }
                continue;
            }
        }
        if constexpr (TF) {  // the table's colour, composited as below: C = sum w * c.rgb (no palette, no 0.5 A + 0.5 G at the end)
            if (COUNT) { n_iter++; n_samp++; if (wave_leader()) w_sample++; }
            if constexpr (LIT) {
                float gx, gy, gz;
                lit_gradient(dx00, dx10, dx01, dx11, c00, c10, c01, c11, c0, c1, fy, fz, fnx, fny, fnz, gx, gy, gz);
                lit_shade(*ld, *lr, gx, gy, gz, tr, tg, tb);
            }
            const float w = (1.0f - A) * a;  // (composite(), written out: the ISA decided -- through the call two COUNT table kernels take two more registers)
            Gr = fmaf(w, tr, Gr); Gg = fmaf(w, tg, Gg); Gb = fmaf(w, tb, Gb);
            A = A + w;
            if (!AHEAD) {
                px = px + sx; py = py + sy; pz = pz + sz;  // :118
                nleft += 1;
            }
            continue;
        }
        float cr, cg, cb;
        palette_cos(a, cr, cg, cb);
        if (COUNT) { n_iter++; n_samp++; if (wave_leader()) w_sample++; }  // (between the cosines and the compositing: the COUNT kernels' registers follow it)
        composite(a, cr, cg, cb, A, Gr, Gg, Gb);  // :112-114
        if (!AHEAD) {
            px = px + sx; py = py + sy; pz = pz + sz;  // :118
            nleft += 1;
        }
    }
    if (AHEAD) asm volatile("" ::"v"(a_d));  // (the last request is consumed on the exit path too)
    r.left = (uint32_t)(-nleft); r.px = px; r.py = py; r.pz = pz; r.A = A; r.Gr = Gr; r.Gg = Gg; r.Gb = Gb;
    return nleft != 0 && A < 0.95f;
}

// The same loop for the fast path without skipping (every trip samples), software-pipelined: the
// position is advanced first and the NEXT trip's cell is requested before this trip's sample is
// evaluated, so the fetch latency overlaps the ~40 VALU instructions of a sample instead of adding
// to them -- it is the lone heavy waves at the tail of a frame that set the frame time.  The f32
// operations on p, A and the colour sums are those of march(), in the same order per variable.
// The request one step past the ray's end is never used.  It reads a real (clamped) table entry while that step is at most 1.5 cells;
// a longer one (dt_scale > 1.5) indexes past the tables, and then only the bounds-checked buffer load keeps the request harmless.
// CELL_LUT: the tables hold cell indices (the skip kernels' copy) instead of byte offsets; `budget` bounds the trips
// (0xffffffff: none) so that the skip kernels can run stretches of it between probing windows.
template <int VOL, bool COUNT, bool CELL_LUT = false, bool TF = false, bool LIT = false>
__device__ __forceinline__ bool march_stream(const VolumeDesc &V, RayState &r, Census &cs, const uint32_t *lut, uint32_t budget = 0xffffffffu,
                                             const TfDesc *tfd = nullptr, const LightDesc *ld = nullptr, const LitRay *lr = nullptr) {
    static_assert(!LIT || TF, "lighting shades the table's colour");
    float px = r.px, py = r.py, pz = r.pz, A = r.A, Gr = r.Gr, Gg = r.Gg, Gb = r.Gb;
    uint32_t left = r.left;
    const float sx = r.sx, sy = r.sy, sz = r.sz;
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    const uint32_t *luty = lut + (V.nx + 3), *lutz = lut + (V.nx + V.ny + 6);
    const __amdgpu_buffer_rsrc_t cells = cell_buffer(V.data, (uint32_t)V.max_off + (1u << V.sh_x));
    if (!(left != 0u && A < 0.95f)) return false;
    const uint32_t lsh = CELL_LUT ? V.sh_x : 0u;
    float fx, fy, fz;
    CellBits<VOL> c0, c1;  // two cell buffers, used alternately (no register copies between trips)
    {
        const float ux = fmaf(px, fnx, -0.5f), uy = fmaf(py, fny, -0.5f), uz = fmaf(pz, fnz, -0.5f);
        fx = __builtin_amdgcn_fractf(ux); fy = __builtin_amdgcn_fractf(uy); fz = __builtin_amdgcn_fractf(uz);
        c0 = request_cell<VOL>(cells, lut, luty, lutz, lsh, ux, uy, uz);
    }
    // one trip: request `nxt` for the advanced position, evaluate `cur`; returns whether the ray goes on
    auto trip = [&](const CellBits<VOL> &cur, CellBits<VOL> &nxt) -> bool {
        if (COUNT) { cs.n_look++; cs.n_iter++; cs.n_samp++; if (wave_leader()) { cs.w_outer++; cs.w_sample++; } }
        px = px + sx; py = py + sy; pz = pz + sz;  // :118
        const float ux = fmaf(px, fnx, -0.5f), uy = fmaf(py, fny, -0.5f), uz = fmaf(pz, fnz, -0.5f);
        nxt = request_cell<VOL>(cells, lut, luty, lutz, lsh, ux, uy, uz);
        float c00, c10, c01, c11;
        float dx00, dx10, dx01, dx11;
        if constexpr (LIT) xlerp_cell_dx<VOL>(cur, fx, c00, c10, c01, c11, dx00, dx10, dx01, dx11);
        else xlerp_cell<VOL>(cur, fx, c00, c10, c01, c11);
        float l0 = fmaf(fy, c10 - c00, c00), l1 = fmaf(fy, c11 - c01, c01);
        float v = fmaf(fz, l1 - l0, l0);
        if constexpr (TF) {
            float cr, cg, cb, a;
            tf_lookup(*tfd, v, cr, cg, cb, a);
            if constexpr (LIT) {
                float gx, gy, gz;
                lit_gradient(dx00, dx10, dx01, dx11, c00, c10, c01, c11, l0, l1, fy, fz, fnx, fny, fnz, gx, gy, gz);
                lit_shade(*ld, *lr, gx, gy, gz, cr, cg, cb);
            }
            composite(a, cr, cg, cb, A, Gr, Gg, Gb);
        } else {
            palette_composite(transfer_alpha<transfer_scale(VOL)>(v), A, Gr, Gg, Gb);
        }
        left -= 1u;  // :101
        fx = __builtin_amdgcn_fractf(ux); fy = __builtin_amdgcn_fractf(uy); fz = __builtin_amdgcn_fractf(uz);
        return left != 0u && A < 0.95f;
    };
    bool alive = true;
    for (;;) {
        if (!trip(c0, c1)) { alive = false; break; }
        if (budget != 0xffffffffu && --budget == 0u) break;
        if (!trip(c1, c0)) { alive = false; break; }
        if (budget != 0xffffffffu && --budget == 0u) break;
    }
    // The last requests are consumed here, on the exit path too: with a use on both sides of the exit
    // branch the compiler cannot sink a request behind it (which would undo the pipelining).
    asm volatile("" ::"v"(c0.v), "v"(c1.v));
    r.left = left; r.px = px; r.py = py; r.pz = pz; r.A = A; r.Gr = Gr; r.Gg = Gg; r.Gb = Gb;
    return alive;
}

// The dense 9^3-brick and quad layouts, software-pipelined the same way: these serve volumes far larger than the caches, where
// every step's loads (four x pairs of a 9^3 brick, one load of a quad) are HBM/fabric latency.  The next trip's loads are
// requested (clamped indices, so always inside the array) before this trip's sample is evaluated.
template <int VOL, bool COUNT>
__device__ __forceinline__ void march_dense_stream(const VolumeDesc &V, RayState &r, Census &cs) {
    static_assert(is_b9(VOL) || is_quads(VOL), "9^3 brick and quad layouts");
    constexpr bool U8 = (VOL == VOL_B9U8 || VOL == VOL_Q8);
    float px = r.px, py = r.py, pz = r.pz, A = r.A, Gr = r.Gr, Gg = r.Gg, Gb = r.Gb;
    uint32_t left = r.left;
    const float sx = r.sx, sy = r.sy, sz = r.sz;
    const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
    if (!(left != 0u && A < 0.95f)) return;
    auto request = [&](float ux, float uy, float uz) -> DenseWords {
        if constexpr (is_b9(VOL)) return b9_request<VOL>(V, cvt_floor_i32(ux), cvt_floor_i32(uy), cvt_floor_i32(uz));
        else return quad_request<VOL>(V, cvt_floor_i32(ux), cvt_floor_i32(uy), cvt_floor_i32(uz));
    };
    float fx, fy, fz;
    DenseWords c0, c1;
    {
        const float ux = fmaf(px, fnx, -0.5f), uy = fmaf(py, fny, -0.5f), uz = fmaf(pz, fnz, -0.5f);
        fx = __builtin_amdgcn_fractf(ux); fy = __builtin_amdgcn_fractf(uy); fz = __builtin_amdgcn_fractf(uz);
        c0 = request(ux, uy, uz);
    }
    auto trip = [&](const DenseWords &cur, DenseWords &nxt) -> bool {
        if (COUNT) { cs.n_look++; cs.n_iter++; cs.n_samp++; if (wave_leader()) { cs.w_outer++; cs.w_sample++; } }
        px = px + sx; py = py + sy; pz = pz + sz;  // :118
        const float ux = fmaf(px, fnx, -0.5f), uy = fmaf(py, fny, -0.5f), uz = fmaf(pz, fnz, -0.5f);
        nxt = request(ux, uy, uz);
        float tp[8], c00, c10, c01, c11;  // tap index dx + 2*dy + 4*dz
        if constexpr (is_b9(VOL)) b9_decode<VOL>(cur, tp);
        else quad_decode<VOL>(cur, tp);
        xlerp_taps(tp, fx, c00, c10, c01, c11);
        palette_composite(transfer_alpha<U8 ? 1 : 0>(lerp_yz(fy, fz, c00, c10, c01, c11)), A, Gr, Gg, Gb);
        left -= 1u;  // :101
        fx = __builtin_amdgcn_fractf(ux); fy = __builtin_amdgcn_fractf(uy); fz = __builtin_amdgcn_fractf(uz);
        return left != 0u && A < 0.95f;
    };
    for (;;) {
        if (!trip(c0, c1)) break;
        if (!trip(c1, c0)) break;
    }
    asm volatile("" ::"v"(c0.a), "v"(c0.b), "v"(c0.c), "v"(c0.d), "v"(c1.a), "v"(c1.b), "v"(c1.c), "v"(c1.d));
    r.left = left; r.px = px; r.py = py; r.pz = pz; r.A = A; r.Gr = Gr; r.Gg = Gg; r.Gb = Gb;
}

// Whole frames in a batched launch: the march covers the active tiles; the tiles behind a frame's active positions hold
// only the clear colour (examples/bonsai/main.rs:41).  They are written by extra blocks at the END of the same grid -- one
// wave clears 512 pixels, 64 consecutive ones per store -- which the dispatcher hands out when the last march waves are
// draining: the stores ride in the launch's tail.  (As blocks of the march proper they were 20 000 waves per C2 frame whose
// only work was a store behind a full wave set-up; as a kernel of their own they cost 2.7 us per frame in series.)
template <int OUT>
__device__ __forceinline__ void clear_inactive_strip(const LaunchDesc &L, uint32_t b, uint32_t lane) {
    const uint32_t strips = (L.ts * L.ts + 511u) / 512u;  // 512-pixel strips per tile
    const uint32_t strip = b % strips; b /= strips;
    const uint32_t j = b % L.clear_max_inactive;
    const uint32_t frame = b / L.clear_max_inactive;
    if (frame >= L.n_frames) return;
    const FrameDesc &d = L.frames[frame];
    const uint32_t n_tiles = L.tiles_x * L.tiles_y, pos = d.pad[0] + j;  // pad[0]: the frame's active tile count
    if (pos >= n_tiles) return;
    const uint32_t tile = L.tile_order[d.order_off + pos];
    const uint32_t tyi = tile / L.tiles_x, txi = tile - tyi * L.tiles_x;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) {  // store k of the wave covers 64 consecutive pixels of the tile's rows
        const uint32_t l = strip * 512u + k * 64u + lane;
        if (l >= L.ts * L.ts) return;
        const uint32_t ly = l / L.ts, lx = l - ly * L.ts;
        const uint32_t x = txi * L.ts + lx, y = tyi * L.ts + ly;
        if (x < L.W && y < L.H) store_pixel<OUT>(L.out, ((size_t)frame * L.H + y) * L.W + x, 0.0f, 0.0f, 0.0f, 1.0f);
    }
}

}  // namespace vk

#include "vk_march_mip.hpp"  // march_mip, march_mip_stream: the loops of the maximum projection, which the kernel body calls under MIP
#include "vk_march_iso.hpp"  // march_iso, march_iso_stream, iso_sample: the loops and the sampler of the isosurface, which the kernel body calls under ISO

namespace vk {

// AHEAD: the probe-ahead trip (march<..., AHEAD>), an instantiation of its own -- it needs six more registers, and the launches that fill the machine keep the leaner kernel
template <int VOL, bool SKIP, bool SAFE, int WALK, bool AHEAD, int OUT, bool COUNT>
__global__ __launch_bounds__(64) void raymarch_naive_kernel(const LaunchDesc L, const VolumeDesc V) {
    constexpr bool TF = false, LIT = false, MIP = false, ISO = false;  // (the table kernels: vk_launch_tf.hip; lit: vk_launch_lit.hip; the maximum projection: vk_launch_mip.hip; the isosurface: vk_launch_iso.hip)
    const TfDesc *tfd = nullptr;
    const LightDesc *ldp = nullptr;
    const IsoDesc *isd = nullptr;
    constexpr bool CLIP = false;  // (no clip box in this family: vk_render.hip refuses the render)
    const ClipDesc *clp = nullptr;
    constexpr bool SHADOW = false;
    const ShadowDesc *shd = nullptr;
    constexpr bool GEOM = false;
    const GeomDesc *gmd = nullptr;
#include "vk_march_kernel_body.hpp"
}

}  // namespace vk
