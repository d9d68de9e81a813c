// vk_march_kernel_body.hpp -- the body of the cell-march kernels, included inside them (no include guard): raymarch_naive_kernel
// (vk_march.hpp), raymarch_tf_kernel (vk_launch_tf.hip), raymarch_lit_kernel (vk_launch_lit.hip), raymarch_mip_kernel
// (vk_launch_mip.hip) and raymarch_iso_kernel (vk_launch_iso.hip).  The including kernel defines the template parameters VOL, SKIP, SAFE,
// WALK, AHEAD, OUT, COUNT, the constants TF (a runtime transfer function: vk_set_transfer_function), LIT (gradient lighting:
// vk_set_lighting), MIP (the maximum-intensity projection: vk_set_projection) and ISO (a first-hit isosurface: vk_set_isosurface),
// `tfd`, its table (nullptr without one; under MIP the window, whose rgba is nullptr for the grey ramp), `ldp`, its lighting (nullptr
// without), `isd`, its isosurface (nullptr without; it brings its own lighting, a runtime flag), the constant CLIP and `clp`, the clip box
// (vk_set_clip_box: the _clip_ kernels of the table, lit, MAX and isosurface families; nullptr in the others, whose rays march the unit
// cube), the constant SHADOW and `shd`, the shadows of the lit isosurface (vk_set_shadows: raymarch_iso_shadow_kernel of
// vk_launch_iso_shadow.hip and its R16_UNORM twin, under ISO alone; false and nullptr in every other kernel), and takes its arguments L
// (LaunchDesc) and V (VolumeDesc) by value.  (Shared textually rather than as an inlined function: that moved the register allocation
// of the existing kernels.)
// Shared by all five families: the block and pixel mapping, the cull, the index tables in LDS, the ray set-up, the wave priority, the
// adaptive-probing policy, the step image, the counters and the trace.  A family's own: its loops -- march / march_stream (vk_march.hpp), or under MIP
// march_mip / march_mip_stream (vk_march_mip.hpp), which take the window's k1, k2 and umax from *tfd and carry the running maximum U in
// RayState::A, or under ISO march_iso / march_iso_stream (vk_march_iso.hpp), which take iso_k from *isd and carry the last sample in
// RayState::A, each a frame of its own around the shared parts of vk_march_parts.hpp; selected at each call site, since a forwarding wrapper
// moved registers -- and what the epilogue makes of the ray's sums: under ISO the refinement of the crossing and
// the shade, once per ray, after the wave's loops have ended.
// The constant GEOM and `gmd` (GeomDesc; nullptr in every other kernel) make the geometry pass of the isosurface (vk_render_geometry; DESIGN.md
// section 18; raymarch_geom_kernel of vk_launch_geom.hip and its R16_UNORM twin): under ISO without SHADOW, the same ray, loops and bisection, and
// an epilogue that stores the crossing, its distance along the ray, the gradient and the sample there in place of a colour.  Every line
// of it sits under `if constexpr (GEOM)`.
    static_assert(is_cell_layout(VOL) || (!SKIP && SAFE), "linear / bricked layouts: no skip map, clamped indices");
    static_assert(SKIP || WALK == WALK_LOOP, "the closed-form walks are variants of the skip kernels");
    static_assert(!AHEAD || (SKIP && !SAFE), "probe ahead: the skip kernels' fast path");
    static_assert(!MIP || (!TF && !LIT && WALK == WALK_LOOP && !AHEAD), "the maximum projection: loops of its own, walking with the loop; the table is looked up in the epilogue");
    static_assert(!MIP || (VOL != VOL_B9U8 && VOL != VOL_B9F16 && VOL != VOL_Q8 && VOL != VOL_QF16), "the maximum projection: LINEAR and cell layouts");
    static_assert(!ISO || (!TF && !LIT && !MIP && WALK == WALK_LOOP && !AHEAD), "the isosurface: loops of its own, walking with the loop; refined and shaded in the epilogue");
    static_assert(!CLIP || TF || MIP || ISO, "the clip box: the table, lit, MAX and isosurface families");
    static_assert(!SHADOW || ISO, "shadows (vk_set_shadows; `shd`, nullptr in the other kernels): the isosurface's epilogue, in kernels of their own (vk_launch_iso_shadow.hip)");
    static_assert(!GEOM || (ISO && !SHADOW && !COUNT), "the geometry pass (vk_render_geometry; `gmd`, nullptr in the other kernels): the isosurface's ray without colour, shadows or counters");
    static_assert(!ISO || (VOL != VOL_B9U8 && VOL != VOL_B9F16 && VOL != VOL_Q8 && VOL != VOL_QF16), "the isosurface: LINEAR and cell layouts");
    if (blockIdx.x >= L.grid_march) {  // wave-uniform
        if constexpr (!GEOM) clear_inactive_strip<OUT>(L, blockIdx.x - L.grid_march, threadIdx.x);  // (the geometry pass is never batched: no such blocks)
        return;
    }
    const uint32_t lb = logical_block(blockIdx.x);
    if (lb >= L.n_blocks) return;  // wave-uniform
    const uint32_t lane = threadIdx.x;
    unsigned long long t_start = 0;
    if (COUNT) t_start = __builtin_amdgcn_s_memrealtime();
    const FrameView fv = frame_view(L, lb);
    const PixelMap pm = map_pixel(L, fv, lane);
    {
        // Screen-space cull (wave-uniform): an 8x8 block wholly outside the projected cube's bounding
        // rectangle (host-computed, padded) holds only misses: clear colour, no ray set-up.
        const int bx0 = pm.x - (int)(lane & 7u), by0 = pm.y - (int)(lane >> 3);
        // ... and so does every block of a tile the box's silhouette cannot reach (the inactive tiles behind the order's
        // active positions: a whole-frame launch covers them too, a partition never launches them)
        if (pm.pos >= fv.n_active || bx0 + 8 <= fv.cull_x0 || bx0 >= fv.cull_x1 || by0 + 8 <= fv.cull_y0 || by0 >= fv.cull_y1) {
            if (!pm.valid) return;
            if constexpr (GEOM) { geom_store(*gmd, L.W, pm.x, pm.y, geom_miss0(), geom_miss1()); return; }  // a culled block, an inactive tile: the miss record
            store_out<OUT>(L, pm, 0.0f, 0.0f, 0.0f);
            if (COUNT && L.steps) L.steps[(size_t)pm.y * L.W + (size_t)pm.x] = 0;
            return;
        }
    }
    constexpr bool USE_LUT = is_cell_layout(VOL) && !SAFE;
    extern __shared__ uint32_t cell_lut[];
    if (USE_LUT) {  // all 64 lanes are still here
        load_cell_luts(V, cell_lut, lane);
        if constexpr (SKIP && !TF && !MIP && !ISO && !AHEAD && (VOL == VOL_P8 || VOL == VOL_P16))  // the corners of the lone-speckle codes (kSpeckleLutBytes; march() decodes with them)
            if (lane < 8u) reinterpret_cast<float4 *>(cell_lut + cell_lut_entries(V.nx, V.ny, V.nz))[lane] = make_float4((lane & 2u) ? 0.0f : 1.0f, (lane & 4u) ? 0.0f : 1.0f, (lane & 1u) ? 0.0f : 1.0f, 0.0f);
        __syncthreads();
    }
    if (!pm.valid) return;

    // --- ray: SURVEY A.1 step 1 (replaces vs_main + rasteriser) ---
    // The set-up's 14 divisions come in two texts.  The short one (vk_exactdiv.hpp) runs first: the compiler's own division chain without its
    // scaling and fix-up instructions -- the same bits while every operand is in range --, the refinement of a divisor shared by its three
    // quotients, and the launch's reciprocals for the two divisions by the image size.  One predicate per lane holds every operand to
    // [kDivLo, kDivHi]: the clip-space point, the far point's offset from the eye (a zero or tiny direction component fails it: 1 / 0 = inf is the
    // reference's, and the generic division's) and its length.  If a single lane fails, or the launch asks for it (LF_SETUP_GENERIC), the
    // whole wave takes the generic text below -- the set-up as it always was -- and nothing of the short one is used.
    const float fxp = (float)pm.x + 0.5f, fyp = (float)pm.y + 0.5f;
    const float eye[3] = {fv.eye[0], fv.eye[1], fv.eye[2]};
    float dir[3], t0, t1;
    [[maybe_unused]] float inv[3];  // short set-up: 1 / dir[i], which dt takes again below
    bool short_setup = !(L.flags & LF_SETUP_GENERIC) && L.W <= kDivConstMax && L.H <= kDivConstMax;  // wave-uniform
    if (short_setup) {
        const float ndcx = div_const(2.0f * fxp, (float)L.W, L.rcp_w) - 1.0f;
        const float ndcy = 1.0f - div_const(2.0f * fyp, (float)L.H, L.rcp_h);
        float q[4];
        mat4_mul_vec4(fv.inv_proj, ndcx, ndcy, 1.0f, 1.0f, q);
        const Recip rq = recip_refine(q[3]);
        const float ex = div_by(q[0], rq) - eye[0], ey = div_by(q[1], rq) - eye[1], ez = div_by(q[2], rq) - eye[2];
        const float len = sqrtf((ex * ex + ey * ey) + ez * ez);
        const Recip rl = recip_refine(len);
        dir[0] = div_by(ex, rl); dir[1] = div_by(ey, rl); dir[2] = div_by(ez, rl);
#pragma unroll
        for (int i = 0; i < 3; i++) inv[i] = div_inrange(1.0f, dir[i]);
        float blo[3] = {0.0f, 0.0f, 0.0f}, bhi[3] = {1.0f, 1.0f, 1.0f};
        if constexpr (CLIP) { for (int i = 0; i < 3; i++) { blo[i] = clp->lo[i]; bhi[i] = clp->hi[i]; } }
        intersect_box_inv(eye, inv, blo, bhi, t0, t1);
        // (len >= every |e|: it bounds them from above, and it is a NaN if anything before it is -- fminf / fmaxf drop a NaN, its own compare does not)
        const float lo = fminf(fminf(fminf(fabsf(q[0]), fabsf(q[1])), fabsf(q[2])), fminf(fminf(fabsf(ex), fabsf(ey)), fminf(fabsf(ez), fabsf(q[3]))));
        const float hi = fmaxf(fmaxf(fabsf(q[0]), fabsf(q[1])), fmaxf(fabsf(q[2]), fabsf(q[3])));
        if (__ballot(!(lo >= kDivLo && hi <= kDivHi && len <= kDivHi)) != 0ull) short_setup = false;
    }
    if (!short_setup) {
        float ndcx = (2.0f * fxp) / (float)L.W - 1.0f;
        float ndcy = 1.0f - (2.0f * fyp) / (float)L.H;
        float q[4];
        mat4_mul_vec4(fv.inv_proj, ndcx, ndcy, 1.0f, 1.0f, q);
        dir[0] = q[0] / q[3] - eye[0]; dir[1] = q[1] / q[3] - eye[1]; dir[2] = q[2] / q[3] - eye[2];
        normalize3(dir[0], dir[1], dir[2]);
        if constexpr (CLIP) intersect_box(eye, dir, clp->lo, clp->hi, t0, t1);  // the clip box (vk_set_clip_box): the family's kernels of their own
        else intersect_box(eye, dir, 0.0f, 1.0f, t0, t1);
    }
    Census cs;
    const bool trip_log = COUNT && L.trace && (L.flags & LF_TRIP_LOG);
    if (trip_log) {  // (the loops of the maximum projection keep no log: such a launch writes neither a log nor stamps)
        cs.log_cap = L.trip_log_cap;
        cs.log = reinterpret_cast<uint32_t *>(L.trace) + (size_t)lb * cs.log_cap;
    }
    // colour is accumulated as G = sum w*cos(phase); C = 0.5*A + 0.5*G at the end (sum w == A)
    float Gr = 0.0f, Gg = 0.0f, Gb = 0.0f, A = 0.0f;
    float Cr = 0.0f, Cg = 0.0f, Cb = 0.0f;
    [[maybe_unused]] float4 geo0, geo1;  // GEOM: the pixel's record, the miss record until the ray hits
    if constexpr (GEOM) { geo0 = geom_miss0(); geo1 = geom_miss1(); }
    if (!(t0 > t1)) {  // :91-93
        t0 = fmaxf(t0, 0.0f);  // :94
        const float fnx = (float)V.nx, fny = (float)V.ny, fnz = (float)V.nz;
        float dtx, dty, dtz;
        if (short_setup) {
            // a power-of-two dimension (wave-uniform, on the scalar unit): 1 / (fn |d|) is |1 / d| (1 / fn) exactly, and 1 / d is at hand
            dtx = is_pow2(V.nx) ? fabsf(inv[0]) * pow2_recip(fnx) : div_inrange(1.0f, fnx * fabsf(dir[0]));
            dty = is_pow2(V.ny) ? fabsf(inv[1]) * pow2_recip(fny) : div_inrange(1.0f, fny * fabsf(dir[1]));
            dtz = is_pow2(V.nz) ? fabsf(inv[2]) * pow2_recip(fnz) : div_inrange(1.0f, fnz * fabsf(dir[2]));
        } else {
            dtx = 1.0f / (fnx * fabsf(dir[0]));
            dty = 1.0f / (fny * fabsf(dir[1]));
            dtz = 1.0f / (fnz * fabsf(dir[2]));
        }
        const float dt = L.dt_scale * fminf(dtx, fminf(dty, dtz));  // :97-99
        float px = eye[0] + t0 * dir[0], py = eye[1] + t0 * dir[1], pz = eye[2] + t0 * dir[2];  // :100
        const float sx = dir[0] * dt, sy = dir[1] * dt, sz = dir[2] * dt;  // :118
        RayState r;
        r.left = min(count_trips(t0, t1, dt), 0x7fffffffu);  // :101
        [[maybe_unused]] const uint32_t left0 = r.left;  // ISO: a hit leaves `left` alone, so a ray that hit with left == left0 hit in its first iteration
        r.px = px; r.py = py; r.pz = pz; r.sx = sx; r.sy = sy; r.sz = sz;
        r.A = 0.0f; r.Gr = 0.0f; r.Gg = 0.0f; r.Gb = 0.0f;  // colour sums: G = sum w*cos(phase); C = A/2 + G/2 (sum w == A); MIP: A is U, the running maximum
        if constexpr (ISO) r.A = __builtin_nanf("");  // ISO: A is the last sample's value; none yet: a NaN meets no threshold (x >= k is false), whatever iso_k is, -inf included
        r.out = (uint32_t)pm.out_index;
        LitRay lr;  // LIT: the ray's light and half vectors (vk_light.hpp; left unset in the other kernels, which never read it)
        if constexpr (LIT) lr = lit_ray(*ldp, dir);
        // (not in the skip kernels: a ray's nominal length says little about its work there -- C2 at 64 orbit frames per launch 0.06509 -> 0.06467 ms without)
        if (!SKIP && (L.flags & LF_WAVE_PRIORITY)) set_wave_priority(true, r.left, fmaxf(fnx, fmaxf(fny, fnz)) / L.dt_scale);
        if constexpr (USE_LUT && !SKIP) {
            if constexpr (ISO) march_iso_stream<VOL, COUNT, false>(V, r, cs, cell_lut, 0xffffffffu, isd->iso_k);
            else if constexpr (MIP) march_mip_stream<VOL, COUNT, false>(V, r, cs, cell_lut, 0xffffffffu, tfd->k1, tfd->k2, tfd->umax);
            else march_stream<VOL, COUNT, false, TF, LIT>(V, r, cs, cell_lut, 0xffffffffu, tfd, ldp, &lr);
        }
        else if constexpr (SKIP) {
            if (L.flags & LF_ADAPTIVE_PROBING) {
                // Adaptive probing (wave-uniform policy, any policy is exact: a sampled empty cell adds +0).  Probe for a
                // window of 16 trips; if fewer than 1 in 8 of the wave's live rays skipped anything in it, the wave is in
                // material that cannot be skipped: run the dense loop -- no distance look-up, and on the fast path
                // software-pipelined -- for a stretch that doubles every time the next window confirms it (64 .. 512
                // trips), then probe again.  Fog pays ~9 % of its trips at the probing price instead of all of them.
                const uint32_t stretch0 = (L.flags & LF_LONG_STRETCHES) ? 256u : 64u;  // the census found (almost) nothing to skip
                uint32_t stretch = stretch0;
                for (;;) {
                    cs.skips = 0;
                    bool alive;
                    if constexpr (ISO) alive = march_iso<VOL, true, SAFE, COUNT, true>(V, r, 16u, cs, USE_LUT ? cell_lut : nullptr, L.walk_cap, L.walk_cap_all, isd->iso_k);
                    else if constexpr (MIP) alive = march_mip<VOL, true, SAFE, COUNT, true>(V, r, 16u, cs, USE_LUT ? cell_lut : nullptr, L.walk_cap, L.walk_cap_all, tfd->k1, tfd->k2, tfd->umax);
                    else alive = march<VOL, true, SAFE, COUNT, true, WALK, false, TF, LIT, !AHEAD>(V, r, 16u, cs, USE_LUT ? cell_lut : nullptr, L.walk_cap, L.walk_cap_all, tfd, ldp, &lr);
                    const unsigned long long live = __ballot(alive);
                    if (live == 0ull) break;
                    if (__popcll(__ballot(alive && cs.skips != 0u)) * 8 >= __popcll(live)) { stretch = stretch0; continue; }
                    if constexpr (ISO && USE_LUT) alive = march_iso_stream<VOL, COUNT, true>(V, r, cs, cell_lut, stretch, isd->iso_k);
                    else if constexpr (ISO) alive = march_iso<VOL, false, SAFE, COUNT, true>(V, r, stretch, cs, nullptr, __builtin_inff(), __builtin_inff(), isd->iso_k);
                    else if constexpr (MIP && USE_LUT) alive = march_mip_stream<VOL, COUNT, true>(V, r, cs, cell_lut, stretch, tfd->k1, tfd->k2, tfd->umax);
                    else if constexpr (MIP) alive = march_mip<VOL, false, SAFE, COUNT, true>(V, r, stretch, cs, nullptr, __builtin_inff(), __builtin_inff(), tfd->k1, tfd->k2, tfd->umax);
                    else if constexpr (USE_LUT) alive = march_stream<VOL, COUNT, true, TF, LIT>(V, r, cs, cell_lut, stretch, tfd, ldp, &lr);
                    else alive = march<VOL, false, SAFE, COUNT, true, WALK_LOOP, false, TF, LIT>(V, r, stretch, cs, nullptr, __builtin_inff(), __builtin_inff(), tfd, ldp, &lr);
                    if (__ballot(alive) == 0ull) break;
                    stretch = min(stretch * 2u, 512u);
                }
            } else if constexpr (ISO) {
                march_iso<VOL, true, SAFE, COUNT, false>(V, r, 0xffffffffu, cs, USE_LUT ? cell_lut : nullptr, L.walk_cap, L.walk_cap_all, isd->iso_k);
            } else if constexpr (MIP) {
                march_mip<VOL, true, SAFE, COUNT, false>(V, r, 0xffffffffu, cs, USE_LUT ? cell_lut : nullptr, L.walk_cap, L.walk_cap_all, tfd->k1, tfd->k2, tfd->umax);
            } else {
                march<VOL, SKIP, SAFE, COUNT, false, WALK, AHEAD, TF, LIT>(V, r, 0xffffffffu, cs, USE_LUT ? cell_lut : nullptr, L.walk_cap, L.walk_cap_all, tfd, ldp, &lr);
            }
        }
        else if constexpr (is_b9(VOL) || is_quads(VOL)) march_dense_stream<VOL, COUNT>(V, r, cs);
        else if constexpr (ISO) march_iso<VOL, false, SAFE, COUNT, false>(V, r, 0xffffffffu, cs, USE_LUT ? cell_lut : nullptr, __builtin_inff(), __builtin_inff(), isd->iso_k);
        else if constexpr (MIP) march_mip<VOL, false, SAFE, COUNT, false>(V, r, 0xffffffffu, cs, USE_LUT ? cell_lut : nullptr, __builtin_inff(), __builtin_inff(), tfd->k1, tfd->k2, tfd->umax);
        else march<VOL, SKIP, SAFE, COUNT, false, WALK_LOOP, false, TF, LIT>(V, r, 0xffffffffu, cs, USE_LUT ? cell_lut : nullptr, __builtin_inff(), __builtin_inff(), tfd, ldp, &lr);
        A = r.A; Gr = r.Gr; Gg = r.Gg; Gb = r.Gb;
        if constexpr (GEOM) {
            // A ray that hit: the wave's hit lanes refine together, whether or not lighting is set (the crossing is what the pass is for), and
            // take the sample at q with its gradient.  The index tables in LDS are still valid, as below.
            if (iso_hit(r.A, isd->iso_k)) {
                const uint32_t *tl = USE_LUT ? cell_lut : nullptr;
                float a = 0.0f;
                if (r.left != left0)  // a hit in the ray's first iteration is not refined
                    a = iso_refine(isd->refine, [&](float m) { return iso_hit(iso_sample<VOL, SKIP, SAFE>(V, tl, iso_back(m, sx, r.px), iso_back(m, sy, r.py), iso_back(m, sz, r.pz)).x, isd->iso_k); });
                const float qx = iso_back(a, sx, r.px), qy = iso_back(a, sy, r.py), qz = iso_back(a, sz, r.pz);
                const IsoSample h = iso_sample<VOL, SKIP, SAFE>(V, tl, qx, qy, qz);
                float gx, gy, gz;
                lit_gradient(h.dx00, h.dx10, h.dx01, h.dx11, h.c00, h.c10, h.c01, h.c11, h.l0, h.l1, h.fy, h.fz, fnx, fny, fnz, gx, gy, gz);
                geo0 = make_float4(qx, qy, qz, geom_distance(qx, qy, qz, eye, dir));
                geo1 = make_float4(gx, gy, gz, h.x);
            }
        } else if constexpr (ISO) {
            // A ray that hit: its colour is the surface's, shaded once.  Only the shade reads the crossing, so the refinement runs
            // under lighting alone: here, after the loops, the wave's hit lanes make the R + 1 dependent fetches together.  The index
            // tables in LDS are still valid (no barrier: nothing has written them since the loops read them).
            if (iso_hit(r.A, isd->iso_k)) {
                float cr = isd->r, cg = isd->g, cb = isd->b;
                if (isd->lit) {
                    const uint32_t *tl = USE_LUT ? cell_lut : nullptr;
                    float a = 0.0f;
                    if (r.left != left0)  // a hit in the ray's first iteration is not refined
                        a = iso_refine(isd->refine, [&](float m) { return iso_hit(iso_sample<VOL, SKIP, SAFE>(V, tl, iso_back(m, sx, r.px), iso_back(m, sy, r.py), iso_back(m, sz, r.pz)).x, isd->iso_k); });
                    const IsoSample h = iso_sample<VOL, SKIP, SAFE>(V, tl, iso_back(a, sx, r.px), iso_back(a, sy, r.py), iso_back(a, sz, r.pz));
                    float gx, gy, gz;
                    lit_gradient(h.dx00, h.dx10, h.dx01, h.dx11, h.c00, h.c10, h.c01, h.c11, h.l0, h.l1, h.fy, h.fz, fnx, fny, fnz, gx, gy, gz);
                    if constexpr (SHADOW) {
                        // the shadow ray (vk_set_shadows): the wave's hit lanes march once more, from the crossing towards the light, through the box the
                        // primary ray marched; a point whose ray hits keeps 1 - strength of its diffuse and specular terms
                        const float qs[3] = {iso_back(a, sx, r.px), iso_back(a, sy, r.py), iso_back(a, sz, r.pz)};
                        const float Ld[3] = {isd->light.lx, isd->light.ly, isd->light.lz};
                        float blo[3] = {0.0f, 0.0f, 0.0f}, bhi[3] = {1.0f, 1.0f, 1.0f};
                        if constexpr (CLIP) { for (int i = 0; i < 3; i++) { blo[i] = clp->lo[i]; bhi[i] = clp->hi[i]; } }
                        const bool dark = iso_shadowed<VOL, SKIP, SAFE>(V, tl, qs, Ld, blo, bhi, L.dt_scale, shd->bias, L.walk_cap, L.walk_cap_all, isd->iso_k);
                        lit_shade(isd->light, lit_ray(isd->light, dir), gx, gy, gz, dark ? shd->k : 1.0f, cr, cg, cb);
                    } else {
                        lit_shade(isd->light, lit_ray(isd->light, dir), gx, gy, gz, cr, cg, cb);
                    }
                }
                Cr = linear_to_srgb(cr); Cg = linear_to_srgb(cg); Cb = linear_to_srgb(cb);
            }
        } else if constexpr (MIP) {
            // the table path's lookup at U, once per ray.  No table: the implicit two-entry grey ramp {(0,0,0), (1,1,1)}, whose lerp
            // fma(U, 1 - 0, 0) is U itself, bit for bit (U is +0 or positive)
            const float U = r.A;
            float cr = U, cg = U, cb = U;
            if (tfd->rgba) {
                const int i = tf_index(U, tfd->imax);
                const float f = U - (float)i;
                const float4 *E = reinterpret_cast<const float4 *>(tfd->rgba);
                const float4 e0 = E[i], e1 = E[i + 1];
                cr = fmaf(f, e1.x - e0.x, e0.x); cg = fmaf(f, e1.y - e0.y, e0.y); cb = fmaf(f, e1.z - e0.z, e0.z);
            }
            Cr = linear_to_srgb(cr); Cg = linear_to_srgb(cg); Cb = linear_to_srgb(cb);
        } else if constexpr (TF) {  // the table's colour sums are the colour
            Cr = linear_to_srgb(Gr); Cg = linear_to_srgb(Gg); Cb = linear_to_srgb(Gb);
        } else {
            Cr = linear_to_srgb(fmaf(0.5f, Gr, 0.5f * A));  // :121-123
            Cg = linear_to_srgb(fmaf(0.5f, Gg, 0.5f * A));
            Cb = linear_to_srgb(fmaf(0.5f, Gb, 0.5f * A));
        }
    }
    if constexpr (GEOM) geom_store(*gmd, L.W, pm.x, pm.y, geo0, geo1);  // no colour: the backbuffer is not touched
    else store_out<OUT>(L, pm, Cr, Cg, Cb);
    if (COUNT) {
        if (L.steps) L.steps[(size_t)pm.y * L.W + (size_t)pm.x] = (L.flags & LF_STEPS_ARE_TRIPS) ? cs.n_look : cs.n_iter;
        if (L.counters) {
            atomicAdd(&L.counters[0], (unsigned long long)cs.n_iter);
            atomicAdd(&L.counters[1], (unsigned long long)cs.n_samp);
            atomicAdd(&L.counters[2], (unsigned long long)cs.w_outer);
            atomicAdd(&L.counters[3], (unsigned long long)cs.w_inner);
            atomicAdd(&L.counters[4], (unsigned long long)cs.w_sample);
            atomicAdd(&L.counters[5], (unsigned long long)cs.n_look);
            if constexpr (SKIP && !TF && !MIP && !ISO) {  // the lone-speckle census of the built-in skip kernels (vk_speckle_census)
                atomicAdd(&L.counters[8], (unsigned long long)cs.w_zero);
                atomicAdd(&L.counters[9], (unsigned long long)cs.n_proven);
            }
        }
        if (L.trace && !trip_log) {  // stamps leave only through this debug buffer
            unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
            atomicMin(&L.trace[4 * (size_t)lb], t_start);
            atomicMax(&L.trace[4 * (size_t)lb + 1], t_end);
            // where the wave ran: HW_ID (wave/simd/cu/sh/se fields) and XCC_ID
            L.trace[4 * (size_t)lb + 2] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                                          ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
            // wave-level work: march-loop trips | skip-walk trips << 20 | sample executions << 40
            atomicAdd(&L.trace[4 * (size_t)lb + 3], (unsigned long long)cs.w_outer | ((unsigned long long)cs.w_inner << 20) | ((unsigned long long)cs.w_sample << 40));
        }
    }
