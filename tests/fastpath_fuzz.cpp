// TEST INFRASTRUCTURE: the audit of the unclamped cell march's dispatch rule, on the CPU, under AddressSanitizer and UBSan
// (tests/test_fastpath_cpu.py builds and runs it; linked with tests/shadow_restatement.c and the oracle's library).
//
// The fast build of the cell march (SAFE = false) reads three per-axis tables that hold voxels [-2, n] and nothing clamps the index: the
// host's rule, vk::cell_march_fast (vk_hostmath.hpp), is all that keeps a ray's indices inside them.  This program replays rays with the
// restatement's own f32 loops (shadow_restatement.c: the primary loop on a volume nothing hits, so every ray runs to the end of its t loop,
// and the shadow walk from random points of the box), records through the restatement's hook every index looked up -- the position the
// probe-ahead trip locates one step past the last sample included, for dt_scale <= 1.25 -- and asserts: wherever the rule says "fast",
// every index lies in [-2, n].  It also holds the tables' entries and the clamped march's offset arithmetic (cell_lut_entry,
// cell_offset_clamped) to the plain 64-bit closed form on every kind of shape the upload accepts, arrays of 4 GiB and more included.
//
//   fastpath_fuzz N SEED                         the fuzz: N random cases, the fixed rows, the self-check, the offsets; "OK (N cases)"
//   fastpath_fuzz rule NX NY NZ EX EY EZ DT FLAGS CELL_BYTES      prints "fast" or "safe": the header's rule, for the Python tests
//   fastpath_fuzz audit NX NY NZ W H DT BLOB     every pixel of a W x H frame under the 144-byte camera in file BLOB: prints
//                                                "min X Y Z max X Y Z trips T rule fast|safe accepted 0|1 overrun 0|1" (T: the longest ray's trips)
//
// The self-check: distance_only_rule() below is the rule without the length of a ray in it: the cell array under 4 GiB, the tables within
// their budget, and 64 ulp(|eye| + 4) < 0.25 / nmax.  On each of the seven fixed rows the audit run against THAT rule must report an
// overrun -- an audit that cannot see a rule that is wrong proves nothing about one that is right.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vk_hostmath.hpp"

extern "C" {
#include "vokselis_oracle.h"
extern void (*shr_lookup_hook)(const float p[3], int ix, int iy, int iz, int ahead);
int shr_render(const vo_camera_uniform *cam, const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, uint32_t W, uint32_t H, uint32_t tx,
               uint32_t ty, uint32_t tw, uint32_t th, float dt_scale, float iso_k, const float *rgb, uint32_t refine, const float *light,
               const float *shadows, const float *box, float *out_rgba, uint32_t *out_steps, float *out_a, uint32_t *out_flags,
               uint32_t *out_sh_iters, float *out_nl);
int shr_shadow_ray(const void *vol, uint32_t nx, uint32_t ny, uint32_t nz, int format, const float q[3], const float L[3], float dt_scale, float bias,
                   float iso_k, uint32_t *n_out);
}

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// ---- the rule that does not know how long a ray is: camera distance only -----------------------------------------------------------------
static bool distance_only_rule(int64_t max_off, uint32_t nx, uint32_t ny, uint32_t nz, const float e[3], uint32_t flags) {
    float reach = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + 4.0f;
    float nmax = (float)std::max(nx, std::max(ny, nz));
    float ulp = std::nextafter(reach, 2.0f * reach) - reach;
    return max_off + 16 < (1ll << 32) && vk::cell_lut_bytes(nx, ny, nz) <= 16384u && 64.0f * ulp < 0.25f / nmax && !(flags & 4u);
}
// check_render's guard (vk_render.hip): a frame it refuses is never marched -- and its loop may never end
static bool render_accepted(uint32_t nx, uint32_t ny, uint32_t nz, const float e[3], float dt_scale) {
    float reach = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + 4.0f;
    float nmax = (float)std::max(nx, std::max(ny, nz));
    float ulp = std::nextafter(reach, 2.0f * reach) - reach;
    return dt_scale > 0.0f && std::isfinite(dt_scale) && dt_scale / nmax >= 8.0f * ulp;
}

// ---- random numbers -------------------------------------------------------------------------------------------------------------
static uint64_t g_rng = 88172645463325252ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
static double uni() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static double uni(double a, double b) { return a + (b - a) * uni(); }
static uint32_t below(uint32_t n) { return (uint32_t)(rnd() % n); }
static uint32_t log_uniform(uint32_t lo, uint32_t hi) {
    const uint32_t v = (uint32_t)std::floor(std::exp(uni(std::log((double)lo), std::log((double)hi + 1.0))));
    return std::min(hi, std::max(lo, v));
}

// ---- what the hook records ------------------------------------------------------------------------------------------------------
struct Seen {
    int lo[3], hi[3];
    bool with_ahead;
    uint64_t lookups;
    void reset(bool ahead) { for (int k = 0; k < 3; k++) { lo[k] = INT32_MAX; hi[k] = INT32_MIN; } with_ahead = ahead; lookups = 0; }
    bool overrun(const uint32_t n[3]) const {
        for (int k = 0; k < 3; k++) if (lookups && (lo[k] < -2 || hi[k] > (int)n[k])) return true;
        return false;
    }
};
static Seen g_seen;
static void hook(const float *, int ix, int iy, int iz, int ahead) {
    if (ahead && !g_seen.with_ahead) return;
    const int i[3] = {ix, iy, iz};
    for (int k = 0; k < 3; k++) { g_seen.lo[k] = std::min(g_seen.lo[k], i[k]); g_seen.hi[k] = std::max(g_seen.hi[k], i[k]); }
    g_seen.lookups++;
}

// ---- a case -----------------------------------------------------------------------------------------------------------------------
struct Case {
    uint32_t n[3];
    vo_camera_uniform cam;
    uint32_t W, H;
    float dt;
};
static const float kNeverHit = INFINITY;  // the isovalue no sample reaches: every primary ray runs its t loop to the end

struct Frame {
    std::vector<float> rgba, a, nl;
    std::vector<uint32_t> steps, flags, sh;
    void size(size_t px) { rgba.assign(4 * px, 0.f); a.assign(px, 0.f); nl.assign(px, 0.f); steps.assign(px, 0u); flags.assign(px, 0u); sh.assign(px, 0u); }
};
// one pixel's primary ray through the restatement; returns its trips
static uint32_t walk_pixel(const Case &c, const uint8_t *vol, Frame &f, uint32_t x, uint32_t y) {
    const float rgb[3] = {1.f, 1.f, 1.f};
    const int rc = shr_render(&c.cam, vol, c.n[0], c.n[1], c.n[2], 0, c.W, c.H, x, y, 1, 1, c.dt, kNeverHit, rgb, 0, nullptr, nullptr, nullptr,
                              f.rgba.data(), f.steps.data(), f.a.data(), f.flags.data(), f.sh.data(), f.nl.data());
    CHECK(rc == 0, "shr_render: %d", rc);
    return f.steps[(size_t)y * c.W + x];
}

// a narrower field of view without a new matrix inverse: NDC x and y scaled by k (a power of two: exact) -- columns 0 and 1 of inv_proj
// by k, rows 0 and 1 of proj_view by 1 / k
static void narrow(vo_camera_uniform &cam, float k) {
    for (int r = 0; r < 4; r++) { cam.inv_proj[r] *= k; cam.inv_proj[4 + r] *= k; }
    for (int c = 0; c < 4; c++) { cam.proj_view[4 * c] /= k; cam.proj_view[4 * c + 1] /= k; }
}

static const float kHalf[3] = {0.5f, 0.5f, 0.5f};
static const double kPi = 3.14159265358979323846;

// the view down axis `ax` from `dist` away, a hundredth of a radian off the axis (the rows' camera for axis 0)
static void camera_down_axis(int ax, float dist, float aspect, vo_camera_uniform &cam) {
    if (ax == 0) vo_camera_uniform_build(dist, 0.02f, (float)(kPi / 2 + 0.01), kHalf, aspect, &cam);
    else if (ax == 2) vo_camera_uniform_build(dist, 0.02f, 0.01f, kHalf, aspect, &cam);
    else vo_camera_uniform_build(dist, (float)(kPi / 2 - 0.02), 0.3f, kHalf, aspect, &cam);
}

struct Verdict { bool fast, distance_only_fast, accepted, overrun; uint32_t max_trips; uint64_t trips; Seen seen; };

// Walk `n_pix` random pixels (n_pix = 0: every pixel) and `n_shadow` secondary rays; returns what was seen, and checks the rule against it.
static Verdict audit(const Case &c, uint32_t n_pix, uint32_t n_shadow, uint64_t trip_budget, int long_axis) {
    uint64_t shadow_trips = 0;  // (the secondary rays have a budget of their own: the primaries of a long case do not use it up)
    Verdict v{};
    const float *eye = c.cam.view_position;
    const int64_t max_off = vk::cell_addr_make(vk::cell_bricks(c.n[0]), vk::cell_bricks(c.n[1]), vk::cell_bricks(c.n[2]), 8).max_off;
    v.fast = vk::cell_march_fast(max_off, c.n[0], c.n[1], c.n[2], eye, c.dt, 0);
    v.distance_only_fast = distance_only_rule(max_off, c.n[0], c.n[1], c.n[2], eye, 0);
    v.accepted = render_accepted(c.n[0], c.n[1], c.n[2], eye, c.dt);
    g_seen.reset(c.dt <= 1.25f);
    if (!v.accepted) { v.seen = g_seen; return v; }  // never marched
    const size_t vox = (size_t)c.n[0] * c.n[1] * c.n[2];
    uint8_t *vol = (uint8_t *)std::calloc(vox, 1);
    CHECK(vol != nullptr, "calloc %zu", vox);
    Frame f;
    f.size((size_t)c.W * c.H);
    shr_lookup_hook = hook;
    const uint32_t total = c.W * c.H;
    for (uint32_t i = 0; i < (n_pix ? n_pix : total) && v.trips < trip_budget; i++) {
        const uint32_t q = n_pix ? below(total) : i;
        const uint32_t t = walk_pixel(c, vol, f, q % c.W, q / c.W);
        v.trips += t;
        v.max_trips = std::max(v.max_trips, t);
    }
    for (uint32_t i = 0; i < n_shadow && shadow_trips < trip_budget; i++) {
        // a point of the box -- inside, or on a face -- and a light direction: any, along an axis, or a hundredth off the long axis
        float q[3], L[3];
        for (int k = 0; k < 3; k++) q[k] = (float)uni();
        if (i % 4 == 1) q[below(3)] = (float)below(2);
        const uint32_t kind = i % 3;
        double d[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
        if (kind == 1) { d[0] = d[1] = d[2] = 0.0; d[below(3)] = below(2) ? 1.0 : -1.0; }
        if (kind == 2) { for (int k = 0; k < 3; k++) d[k] = uni(-0.02, 0.02); d[long_axis] = below(2) ? 1.0 : -1.0; }
        const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(len > 1e-3)) continue;
        for (int k = 0; k < 3; k++) L[k] = (float)(d[k] / len);
        uint32_t t = 0;
        const int rc = shr_shadow_ray(vol, c.n[0], c.n[1], c.n[2], 0, q, L, c.dt, (float)uni(0.0, 4.0), kNeverHit, &t);
        CHECK(rc == 0, "shr_shadow_ray: %d", rc);
        v.trips += t;
        shadow_trips += t;
        v.max_trips = std::max(v.max_trips, t);
    }
    shr_lookup_hook = nullptr;
    std::free(vol);
    v.seen = g_seen;
    v.overrun = g_seen.overrun(c.n);
    // THE assertion: a frame the rule sends down the unclamped build looks up nothing outside the tables
    CHECK(!(v.fast && v.overrun), "rule says fast, dims %u x %u x %u, eye (%g %g %g), dt %g: indices x [%d, %d] y [%d, %d] z [%d, %d], longest ray %u trips",
          c.n[0], c.n[1], c.n[2], eye[0], eye[1], eye[2], c.dt, g_seen.lo[0], g_seen.hi[0], g_seen.lo[1], g_seen.hi[1], g_seen.lo[2], g_seen.hi[2], v.max_trips);
    return v;
}

// ---- the seven fixed rows: 16 x 8 frames down the long x axis of an nx x 4 x 4 volume ------------------------------------------------------------------
struct Row { uint32_t nx; float dist, dt; };
static const Row kRows[7] = {{2048, 3.4f, 0.25f}, {2048, 3.4f, 0.05f}, {4000, 3.4f, 0.25f}, {4000, 2.0f, 0.1f}, {4000, 3.4f, 0.1f}, {4000, 2.0f, 0.05f}, {4000, 3.4f, 0.05f}};

static void fixed_rows() {
    for (const Row &r : kRows) {
        Case c{};
        c.n[0] = r.nx; c.n[1] = 4; c.n[2] = 4;
        c.W = 16; c.H = 8; c.dt = r.dt;
        vo_camera_uniform_build(r.dist, 0.02f, (float)(kPi / 2 + 0.01), kHalf, 2.0f, &c.cam);
        const Verdict v = audit(c, 0, 0, ~0ull, 0);
        // the self-check: the distance-only rule takes the unclamped build here, and the audit sees the overrun
        CHECK(v.accepted && v.distance_only_fast && v.overrun && v.seen.hi[0] > (int)r.nx, "self-check, %u x 4 x 4 from %g at dt %g: distance-only rule fast %d, overrun %d, x up to %d",
              r.nx, r.dist, r.dt, (int)v.distance_only_fast, (int)v.overrun, v.seen.hi[0]);
        CHECK(!v.fast, "the rule still says fast");
        std::printf("row %u x 4 x 4, camera %.1f away, dt %.2f: longest ray %u trips, x index up to %d (table holds up to %u); distance-only rule fast, the rule safe\n",
                    r.nx, r.dist, r.dt, v.max_trips, v.seen.hi[0], r.nx);
    }
}

// ---- the random domain ----------------------------------------------------------------------------------------------------------------
static const uint32_t kVoxelCap = 1u << 24;  // the replay's volume is allocated: 16 MiB at the most

static void random_dims(uint32_t trial, uint32_t n[3], int &long_axis) {
    long_axis = (int)(trial % 3);
    const uint32_t kind = (trial / 3) % 5;
    for (;;) {
        if (kind == 0) {  // sums on both sides of the tables' budget: 4087 fits, 4088 does not
            const uint32_t sum = 4085u + below(6), a = 1u + below(8), b = 1u + below(8);
            n[long_axis] = sum - a - b; n[(long_axis + 1) % 3] = a; n[(long_axis + 2) % 3] = b;
        } else if (kind == 1) {  // the limit's dims: nmax = 32, 256, 2048, 4000
            static const uint32_t nm[4] = {32, 256, 2048, 4000};
            n[long_axis] = nm[below(4)];
            n[(long_axis + 1) % 3] = log_uniform(1, std::min(n[long_axis], 64u)); n[(long_axis + 2) % 3] = log_uniform(1, std::min(n[long_axis], 64u));
        } else {
            for (int k = 0; k < 3; k++) n[k] = log_uniform(1, 4200);
            uint32_t m = 0;
            for (int k = 1; k < 3; k++) if (n[k] > n[m]) m = k;
            std::swap(n[m], n[long_axis]);
        }
        if ((uint64_t)n[0] * n[1] * n[2] <= kVoxelCap) return;
    }
}

static void random_camera(uint32_t trial, const uint32_t n[3], int long_axis, Case &c) {
    c.W = 24 + below(41); c.H = 16 + below(33);
    const float aspect = (float)c.W / (float)c.H;
    const uint32_t kind = trial % 7;
    float target[3] = {0.5f, 0.5f, 0.5f};
    if (kind == 0) vo_camera_uniform_build((float)uni(0.7, 2.5), (float)uni(-1.4, 1.4), (float)uni(0, 6.28), target, aspect, &c.cam);  // orbit
    else if (kind == 1) {  // eye inside the volume
        for (int k = 0; k < 3; k++) target[k] = (float)uni(0.3, 0.7);
        vo_camera_uniform_build((float)uni(0.05, 0.4), (float)uni(-1.0, 1.0), (float)uni(0, 6.28), target, aspect, &c.cam);
    } else if (kind == 2) vo_camera_uniform_build(1.5f, 0.0f, (float)below(4) * 1.5707963f, target, 1.0f, &c.cam);  // axis-aligned
    else if (kind == 3) {  // grazing a face
        target[1] = below(2) ? 0.02f : 0.98f;
        vo_camera_uniform_build(1.2f, (float)uni(-0.05, 0.05), (float)uni(0, 6.28), target, aspect, &c.cam);
    } else if (kind == 4) camera_down_axis(long_axis, (float)uni(0.6, 3.5), aspect, c.cam);  // down the long axis, near
    else {
        // far: |eye| + 4 on both sides of the binade edge at which the rule's ulp doubles -- 1024, 128, 16, 8 are the edges the limit sits
        // on for nmax = 32, 256, 2048, 4000 -- down the long axis or from anywhere, through a field narrowed to the box
        static const float edge[4] = {1024.f, 128.f, 16.f, 8.f};
        const uint32_t nmax = std::max(n[0], std::max(n[1], n[2]));
        float e = (kind == 5) ? edge[nmax <= 32 ? 0 : (nmax <= 256 ? 1 : (nmax <= 2048 ? 2 : 3))] : edge[below(4)];
        // ... those four are the distance-only limits; every other time the edge is THIS rule's for the case's dims and dt_scale: the
        // power of two from which on cell_march_fast says "safe" (none where its rays are too long at every distance)
        if (below(2)) {
            const int64_t max_off = vk::cell_addr_make(vk::cell_bricks(n[0]), vk::cell_bricks(n[1]), vk::cell_bricks(n[2]), 8).max_off;
            float own = 8.0f;
            const float at0[3] = {0.f, 0.f, 0.f};
            if (vk::cell_march_fast(max_off, n[0], n[1], n[2], at0, c.dt, 0)) {
                for (;;) {
                    const float at[3] = {own - 4.0f, 0.f, 0.f};
                    if (own >= 65536.0f || !vk::cell_march_fast(max_off, n[0], n[1], n[2], at, c.dt, 0)) break;
                    own *= 2.0f;
                }
                e = own;
            }
        }
        const float dist = std::max(0.9f, e - 4.0f + (float)uni(-1.0, 1.0) * std::min(1.0f, e / 16.0f));
        if (below(2)) camera_down_axis(long_axis, dist, aspect, c.cam);
        else vo_camera_uniform_build(dist, (float)uni(-1.2, 1.2), (float)uni(0, 6.28), target, aspect, &c.cam);
        float k = 1.0f;
        while (k * dist > 1.5f) k *= 0.5f;
        narrow(c.cam, k);
    }
}

static void fuzz(uint32_t n_cases) {
    uint32_t n_fast = 0, n_safe = 0, n_refused = 0, n_distance_only_overruns = 0, longest = 0;
    uint64_t trips = 0;
    for (uint32_t trial = 0; trial < n_cases; trial++) {
        Case c{};
        int long_axis = 0;
        random_dims(trial, c.n, long_axis);
        // dt_scale over what check_render accepts (any finite dt > 0 that still advances t), at up to about 1e5 trips per ray
        const uint32_t nmax = std::max(c.n[0], std::max(c.n[1], c.n[2]));
        const double dt_lo = std::max(0.012, (double)nmax / 1.0e5);
        c.dt = (float)std::exp(uni(std::log(dt_lo), std::log(4.0)));
        if (trial % 11 == 0) c.dt = 1.25f;   // the last dt_scale that keeps the probe-ahead trip
        if (trial % 11 == 5) c.dt = 1.0f;
        random_camera(trial, c.n, long_axis, c);  // (after dt_scale: the far cameras sit at the rule's own edge for it)
        const Verdict v = audit(c, 48, 24, 1500000ull, long_axis);
        trips += v.trips;
        longest = std::max(longest, v.max_trips);
        if (!v.accepted) n_refused++;
        else if (v.fast) n_fast++;
        else n_safe++;
        if (v.accepted && v.distance_only_fast && v.overrun) n_distance_only_overruns++;
    }
    std::printf("fuzz: %u fast, %u safe, %u refused by the render's dt guard; %" PRIu64 " trips replayed, longest ray %u; the distance-only rule overran on %u cases\n",
                n_fast, n_safe, n_refused, trips, longest, n_distance_only_overruns);
    CHECK(n_fast * 5 >= n_cases && n_safe * 5 >= n_cases, "both sides of the rule: %u fast, %u safe of %u", n_fast, n_safe, n_cases);
}

// ---- the tables and the clamped offset against the 64-bit closed form -------------------------------------------------------------------
// the cell with low-corner voxel (ix, iy, iz), i in [-1, n - 1]: physical brick (i >> 2) + 1, position i & 3
static uint64_t cell_index_closed(uint64_t nbx, uint64_t nby, int ix, int iy, int iz) {
    const uint64_t bx = (uint64_t)((ix >> 2) + 1), by = (uint64_t)((iy >> 2) + 1), bz = (uint64_t)((iz >> 2) + 1);
    return 64u * ((bz * nby + by) * nbx + bx) + 16u * (uint64_t)(iz & 3) + 4u * (uint64_t)(iy & 3) + (uint64_t)(ix & 3);
}
static int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static uint32_t g_shapes = 0, g_big = 0;
static void check_shape(uint32_t nx, uint32_t ny, uint32_t nz) {
    const uint32_t nbx = vk::cell_bricks(nx), nby = vk::cell_bricks(ny), nbz = vk::cell_bricks(nz);
    const uint64_t n_bricks = (uint64_t)nbx * nby * nbz, n_cells = n_bricks * 64u;
    if (n_bricks >= (1ull << 31) || n_cells >= (1ull << 32)) return;  // the upload refuses it
    g_shapes++;
    const uint32_t n[3] = {nx, ny, nz};
    for (uint32_t cell_bytes : {8u, 16u}) {  // u8 cells; pairs, u16 and f16 cells
        const vk::CellAddr A = vk::cell_addr_make(nbx, nby, nbz, cell_bytes);
        CHECK(A.max_off == (int64_t)((n_cells - 1) * cell_bytes), "max_off");
        if (A.max_off + 16 >= (1ll << 32)) g_big++;
        for (uint32_t s = 0; s < 27 + 24 + 64; s++) {
            int i[3];
            for (int k = 0; k < 3; k++) {
                if (s < 27) { const uint32_t d = (s / (k == 0 ? 1 : (k == 1 ? 3 : 9))) % 3; i[k] = d == 0 ? -1 : (d == 1 ? (int)n[k] - 1 : (int)(n[k] / 2)); }  // corners, edges, faces
                else if (s < 51) i[k] = below(2) ? (below(2) ? -1 : (int)n[k] - 1) : (int)below(n[k] + 1) - 1;                                       // on an edge
                else i[k] = (int)below(n[k] + 1) - 1;
            }
            const uint64_t want = cell_index_closed(nbx, nby, i[0], i[1], i[2]);
            CHECK(want < n_cells, "closed form");
            const int64_t got = vk::cell_offset_clamped(A.kz, A.c0, A.max_off, A.kx, A.ky, A.sh_x, A.sh_y, A.sh_z, i[0], i[1], i[2]);
            CHECK(got == (int64_t)(want * cell_bytes), "offset of voxel (%d %d %d) in %u x %u x %u, %u-byte cells: %" PRId64 " for %" PRIu64, i[0], i[1], i[2], nx, ny, nz,
                  cell_bytes, got, want * cell_bytes);
            // the tables: entry i + 2 for i in [-2, n], the outer two clamped; their sum is the cell's index (32 bits: every index is below 2^32)
            if (cell_bytes == 8) {
                int j[3];
                for (int k = 0; k < 3; k++) j[k] = s < 27 ? (i[k] == -1 ? -2 : (i[k] == (int)n[k] - 1 ? (int)n[k] : i[k])) : i[k];  // the padding entries too
                const uint32_t sum = vk::cell_lut_entry((uint32_t)(j[0] + 2), nx, ny, nz, nbx, nby) + vk::cell_lut_entry(nx + 3u + (uint32_t)(j[1] + 2), nx, ny, nz, nbx, nby) +
                                     vk::cell_lut_entry(nx + ny + 6u + (uint32_t)(j[2] + 2), nx, ny, nz, nbx, nby);
                const uint64_t at = cell_index_closed(nbx, nby, clampi(j[0], -1, (int)nx - 1), clampi(j[1], -1, (int)ny - 1), clampi(j[2], -1, (int)nz - 1));
                CHECK(sum == (uint32_t)at, "tables at voxel (%d %d %d) in %u x %u x %u: %u for %" PRIu64, j[0], j[1], j[2], nx, ny, nz, sum, at);
            }
        }
    }
    for (uint32_t e = nx + ny + nz + 9u; e < vk::cell_lut_entries(nx, ny, nz); e++) CHECK(vk::cell_lut_entry(e, nx, ny, nz, nbx, nby) == 0u, "padding");
}

static void offsets() {
    // a flat u16 volume whose by * ky passes 2^31 (5800 x 5800 x 4), flat and line shapes up to the dims' limit (8192), shapes at the 2^32-cell limit, and random ones
    check_shape(5800, 5800, 4);
    static const uint32_t edge[] = {1, 2, 3, 4, 5, 8, 9, 4079, 4080, 5800, 8191, 8192};
    for (uint32_t a : edge) for (uint32_t b : edge) for (uint32_t c : edge) check_shape(a, b, c);
    for (uint32_t a = 1600; a <= 1640; a += 4) check_shape(a, a, a);            // about 1600^3: the last cubes the cell layouts hold
    for (uint32_t trial = 0; trial < 3000; trial++) {
        uint32_t n[3];
        for (int k = 0; k < 3; k++) n[k] = log_uniform(1, 8192);
        if (trial % 3 == 0) n[below(3)] = log_uniform(1, 8);                    // flat
        if (trial % 3 == 1) { const uint32_t l = below(3); n[(l + 1) % 3] = log_uniform(1, 8); n[(l + 2) % 3] = log_uniform(1, 8); }  // a line
        check_shape(n[0], n[1], n[2]);
    }
    CHECK(g_shapes > 2000 && g_big > 200, "shapes %u, of 4 GiB and more %u", g_shapes, g_big);
    std::printf("offsets: %u accepted shapes, %u arrays of 4 GiB and more: the clamped offset and the tables equal the 64-bit closed form\n", g_shapes, g_big);
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "rule")) {
        CHECK(argc == 11, "rule NX NY NZ EX EY EZ DT FLAGS CELL_BYTES");
        const uint32_t n[3] = {(uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4])};
        const float eye[3] = {std::strtof(argv[5], nullptr), std::strtof(argv[6], nullptr), std::strtof(argv[7], nullptr)};
        const vk::CellAddr A = vk::cell_addr_make(vk::cell_bricks(n[0]), vk::cell_bricks(n[1]), vk::cell_bricks(n[2]), (uint32_t)std::atoi(argv[10]));
        std::printf("%s\n", vk::cell_march_fast(A.max_off, n[0], n[1], n[2], eye, std::strtof(argv[8], nullptr), (uint32_t)std::strtoul(argv[9], nullptr, 0)) ? "fast" : "safe");
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "audit")) {
        CHECK(argc == 9, "audit NX NY NZ W H DT BLOB");
        Case c{};
        for (int k = 0; k < 3; k++) c.n[k] = (uint32_t)std::atoi(argv[2 + k]);
        c.W = (uint32_t)std::atoi(argv[5]); c.H = (uint32_t)std::atoi(argv[6]); c.dt = std::strtof(argv[7], nullptr);
        FILE *fp = std::fopen(argv[8], "rb");
        CHECK(fp && std::fread(&c.cam, 1, sizeof c.cam, fp) == sizeof c.cam, "camera blob %s", argv[8]);
        std::fclose(fp);
        const Verdict v = audit(c, 0, 0, ~0ull, 0);
        std::printf("min %d %d %d max %d %d %d trips %u rule %s accepted %d overrun %d\n", v.seen.lo[0], v.seen.lo[1], v.seen.lo[2], v.seen.hi[0], v.seen.hi[1], v.seen.hi[2],
                    v.max_trips, v.fast ? "fast" : "safe", (int)v.accepted, (int)v.overrun);
        return 0;
    }
    const uint32_t n_cases = argc > 1 ? (uint32_t)std::atoi(argv[1]) : 200u;
    if (argc > 2) g_rng = std::strtoull(argv[2], nullptr, 0) | 1ull;
    offsets();
    fixed_rows();
    fuzz(n_cases);
    std::printf("OK (%u cases)\n", n_cases);
    return 0;
}
