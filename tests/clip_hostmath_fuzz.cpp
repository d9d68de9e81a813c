// TEST INFRASTRUCTURE: the host geometry of vokselis_amd/csrc/vk_hostmath.hpp under a clip box (vk_set_clip_box) -- cull_rect_wh,
// cull_hull_wh, tile_cull_wh / tile_is_inactive and tile_order with their trailing box -- built by plain g++ with
// -fsanitize=address,undefined and fuzzed on the CPU, as tests/hostmath_fuzz.cpp does for the unit cube.  Every table is a std::vector of
// exactly the size the library allocates.
//
//   unit box:  rectangle, hull, active set and order of the box (0,0,0)-(1,1,1) are those of the calls without a box, value for value.
//   order:     under a box tile_order is a permutation with the active tiles in front and the inactive ones in index order, order_pos its
//              inverse, and its active set is tile_is_inactive's decision.
//   cull:      NO pixel whose ray (cast in double) hits the box lies in an inactive tile or outside the box's cull rectangle: the tile's
//              corner pixels, its centre and random pixels of it -- for boxes from a sliver to the whole cube and cameras around the cube,
//              inside the cube, inside the box, axis-aligned (edge-on), grazing a box face, with box corners behind the eye.
//   monotone:  a tile that is inactive without a box is inactive under every box; the box's rectangle lies inside the cube's.
//
// usage: clip_hostmath_fuzz <cases> <seed>; prints "clip_hostmath_fuzz: OK (<cases> cases)" and exits 0, or the first failures and exits 1.
#include "vk_hostmath.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace vk;

static uint64_t state;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static double unit() { return (double)(rnd() >> 11) / 9007199254740992.0; }
static uint32_t pick(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rnd() % (uint64_t)(hi - lo + 1)); }

static long g_bad = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (g_bad++ < 20) { printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                 \
    } while (0)

// ---- a camera blob: eye = target - zoom (sin yaw cos pitch, sin pitch, cos yaw cos pitch), look_at_rh, perspective_rh(pi/2, aspect, .1, 100) ----
struct Cam { float blob[36]; double eye[3]; };
static void mat_mul(const double a[16], const double b[16], double o[16]) {  // column-major
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) { double s = 0; for (int k = 0; k < 4; k++) s += a[k * 4 + r] * b[c * 4 + k]; o[c * 4 + r] = s; }
}
static bool make_camera(double zoom, double pitch, double yaw, const double tgt[3], double aspect, Cam &out) {
    const double pc = cos(pitch);
    const double eye[3] = {tgt[0] - zoom * sin(yaw) * pc, tgt[1] - zoom * sin(pitch), tgt[2] - zoom * cos(yaw) * pc};
    double f[3] = {tgt[0] - eye[0], tgt[1] - eye[1], tgt[2] - eye[2]};
    const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (!(fl > 1e-9)) return false;
    for (double &v : f) v /= fl;
    double s[3] = {-f[2], 0.0, f[0]};  // cross(f, up), up = (0, 1, 0)
    const double sl = sqrt(s[0] * s[0] + s[2] * s[2]);
    if (!(sl > 1e-9)) return false;
    for (double &v : s) v /= sl;
    const double u[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
    const double V[16] = {s[0], u[0], -f[0], 0, s[1], u[1], -f[1], 0, s[2], u[2], -f[2], 0,
                          -(s[0] * eye[0] + s[1] * eye[1] + s[2] * eye[2]), -(u[0] * eye[0] + u[1] * eye[1] + u[2] * eye[2]), f[0] * eye[0] + f[1] * eye[1] + f[2] * eye[2], 1};
    // the view is rigid and the projection sparse: both inverses in closed form
    const double Vi[16] = {s[0], s[1], s[2], 0, u[0], u[1], u[2], 0, -f[0], -f[1], -f[2], 0, eye[0], eye[1], eye[2], 1};
    const double h = 1.0, w = h / aspect, zn = 0.1, zf = 100.0, r = zf / (zn - zf);
    const double P[16] = {w, 0, 0, 0, 0, h, 0, 0, 0, 0, r, -1, 0, 0, r * zn, 0};
    const double Pi[16] = {1 / w, 0, 0, 0, 0, 1 / h, 0, 0, 0, 0, 0, 1 / (r * zn), 0, 0, -1, 1 / zn};
    double PV[16], inv[16];
    mat_mul(P, V, PV);
    mat_mul(Vi, Pi, inv);
    out.blob[0] = (float)eye[0]; out.blob[1] = (float)eye[1]; out.blob[2] = (float)eye[2]; out.blob[3] = 1.0f;
    for (int i = 0; i < 16; i++) { out.blob[4 + i] = (float)PV[i]; out.blob[20 + i] = (float)inv[i]; }
    for (float v : out.blob) if (!std::isfinite(v)) return false;
    for (int k = 0; k < 3; k++) out.eye[k] = out.blob[k];
    return true;
}

// ---- boxes: f32 bounds with 0 <= lo < hi <= 1 (what vk_set_clip_box accepts), held in double as the library holds them ----
static ClipBox random_box(int kind) {
    ClipBox b;
    for (int k = 0; k < 3; k++) {
        float lo = (float)unit(), hi = (float)unit();
        if (hi < lo) std::swap(lo, hi);
        if (kind == 1 && k == (int)(rnd() % 3)) { lo = 0.3f + 0.4f * (float)unit(); hi = lo + 0.02f * (float)unit() + 1e-4f; }  // a slab
        if (kind == 2) { lo = (float)pick(0, 6) / 8.0f; hi = lo + (float)pick(1, 8 - (uint32_t)(lo * 8.0f)) / 8.0f; }      // on brick boundaries
        if (kind == 3 && (rnd() & 1)) { lo = 0.0f; hi = 1.0f; }                                                          // a half-space or the cube
        if (!(hi > lo)) hi = std::nextafter(lo, 2.0f);
        if (hi > 1.0f) { hi = 1.0f; if (!(lo < hi)) lo = 0.5f; }
        b.lo[k] = lo; b.hi[k] = hi;
    }
    return b;
}

static int g_kinds[6];
static bool random_camera(double aspect, const ClipBox &box, Cam &c) {
    const int kind = (int)(rnd() % 6);
    double tgt[3] = {0.5, 0.5, 0.5}, mid[3];
    for (int k = 0; k < 3; k++) mid[k] = 0.5 * (box.lo[k] + box.hi[k]);
    double zoom = 0.3 + unit() * 3.0, pitch = (unit() - 0.5) * 3.0, yaw = unit() * 6.2831853;
    if (kind == 1) { for (int k = 0; k < 3; k++) tgt[k] = unit(); zoom = 0.05 + unit() * 0.4; }                             // eye inside the cube (often outside the box)
    if (kind == 2) { for (int k = 0; k < 3; k++) tgt[k] = mid[k]; zoom = 0.4 * std::min({box.hi[0] - box.lo[0], box.hi[1] - box.lo[1], box.hi[2] - box.lo[2]}); }  // eye inside the box
    if (kind == 3) { pitch = 0.0; yaw = (double)(rnd() % 4) * 1.5707963; for (int k = 0; k < 3; k++) tgt[k] = mid[k]; }     // axis-aligned: an edge-on hull
    if (kind == 4) {                                                                                                        // grazing a box face: the eye in the face's plane
        const int a = (int)(rnd() % 3);
        for (int k = 0; k < 3; k++) tgt[k] = mid[k];
        tgt[a] = (rnd() & 1) ? box.hi[a] : box.lo[a];
        if (a == 1) pitch = 0.0; else { pitch = (unit() - 0.5) * 1.0; yaw = (a == 0 ? 0.0 : 1.5707963) + ((rnd() & 1) ? 3.1415927 : 0.0); }
    }
    if (kind == 5) { for (int k = 0; k < 3; k++) tgt[k] = mid[k] + (unit() - 0.5) * 2.0; zoom = 0.3 + unit(); }             // looking past the box; corners behind the eye
    g_kinds[kind]++;
    return make_camera(zoom, pitch, yaw, tgt, aspect, c);
}

// does the ray through pixel centre (px, py) hit the box?  In double, strictly: by a margin in t (a grazing ray may go either way in the
// kernel's float arithmetic, and either way its pixel is clear-coloured)
static bool ray_hits(const Cam &c, const ClipBox &box, uint32_t W, uint32_t H, double px, double py) {
    const float *m = c.blob + 20;
    double e[3], d[3];
    const double X = 2.0 * px / W - 1.0, Y = 1.0 - 2.0 * py / H;
    const double qw = m[3] * X + m[7] * Y + m[11] + m[15];
    for (int k = 0; k < 3; k++) { e[k] = c.blob[k]; d[k] = (m[k] * X + m[4 + k] * Y + m[8 + k] + m[12 + k]) / qw - e[k]; }
    double t0 = -1e300, t1 = 1e300;
    for (int k = 0; k < 3; k++) {
        const double inv = 1.0 / d[k], ta = (box.lo[k] - e[k]) * inv, tb = (box.hi[k] - e[k]) * inv;
        if (ta != ta || tb != tb) return false;  // (0 * inf: the ray lies in a face plane; not a case to decide here)
        t0 = std::max(t0, std::min(ta, tb)); t1 = std::min(t1, std::max(ta, tb));
    }
    return t1 > std::max(t0, 0.0) + 1e-6;
}

static long g_inactive_checked = 0, g_fewer = 0, g_eye_in_box = 0, g_eye_in_cube = 0, g_no_cull = 0;

static void fuzz_case(int round) {
    static const uint32_t tss[] = {8, 16, 24, 32, 40, 64, 128};
    const uint32_t ts = tss[rnd() % 7];
    uint32_t W = pick(1, 700), H = pick(1, 500);
    if (rnd() % 4 == 0) { W = (W / ts + 1) * ts; H = (H / ts + 1) * ts; }
    const ClipBox box = round % 16 == 0 ? ClipBox() : random_box((int)(rnd() % 4));
    Cam cam;
    if (!random_camera((double)W / H, box, cam)) return;
    bool in_box = true, in_cube = true;
    for (int k = 0; k < 3; k++) { in_box = in_box && cam.eye[k] > box.lo[k] && cam.eye[k] < box.hi[k]; in_cube = in_cube && cam.eye[k] > 0.0 && cam.eye[k] < 1.0; }
    g_eye_in_box += in_box; g_eye_in_cube += in_cube && !in_box;
    const uint32_t dims[3] = {pick(1, 512), pick(1, 512), pick(1, 512)};
    const uint32_t tx = (W + ts - 1) / ts, ty = (H + ts - 1) / ts;
    const size_t n = (size_t)tx * ty;
    const int G = (int)pick(1, 3);
    std::vector<uint32_t> order(n, 0xffffffffu), pos(n, 0xffffffffu), order0(n, 0xffffffffu), pos0(n, 0xffffffffu);
    uint32_t n_active = 0, n_active0 = 0;
    tile_order(W, H, dims, cam.blob, kModeNaive, 0, 0, W, H, ts, order.data(), pos.data(), n_active, G, box);
    tile_order(W, H, dims, cam.blob, kModeNaive, 0, 0, W, H, ts, order0.data(), pos0.data(), n_active0, G);
    // a permutation, its inverse, the active tiles in front, the inactive ones in index order
    CHECK(n_active <= n, "n_active %u of %zu", n_active, n);
    std::vector<char> seen(n, 0);
    for (size_t q = 0; q < n; q++) {
        CHECK(order[q] < n, "order[%zu] = %u of %zu tiles", q, order[q], n);
        if (order[q] >= n) return;
        CHECK(!seen[order[q]], "tile %u twice in the order", order[q]);
        seen[order[q]] = 1;
        CHECK(pos[order[q]] == q, "order_pos is not the inverse at %zu", q);
    }
    for (size_t q = n_active; q + 1 < n; q++) CHECK(order[q] < order[q + 1], "inactive tiles out of index order at %zu", q);
    // a box never activates a tile
    CHECK(n_active <= n_active0, "%u active tiles under the box, %u without", n_active, n_active0);
    g_fewer += n_active < n_active0;
    for (size_t t = 0; t < n; t++) CHECK(!(pos0[t] >= n_active0) || pos[t] >= n_active, "tile %zu is inactive without a box and active under one", t);
    // the decision, as vk_tiles_active_clip and the kernels' per-block cull take it
    TileCull cull;
    tile_cull_wh(W, H, cam.blob, kModeNaive, box, cull);
    int32_t cr[4], cr0[4];
    cull_rect_wh(W, H, cam.blob, kModeNaive, cr, box);
    cull_rect_wh(W, H, cam.blob, kModeNaive, cr0);
    CHECK(cr[0] >= 0 && cr[1] >= 0 && cr[2] <= (int32_t)W && cr[3] <= (int32_t)H, "cull rectangle outside the frame");
    CHECK(memcmp(cr, cull.cr, sizeof cr) == 0, "tile_cull_wh's rectangle is not cull_rect_wh's");
    CHECK((cr[0] >= cr0[0] && cr[1] >= cr0[1] && cr[2] <= cr0[2] && cr[3] <= cr0[3]) || cr[0] >= cr[2] || cr[1] >= cr[3], "the box's rectangle leaves the cube's");
    g_no_cull += cr[0] == 0 && cr[1] == 0 && cr[2] == (int32_t)W && cr[3] == (int32_t)H && cull.hull.n == 0;
    CullHull hull;
    cull_hull_wh(W, H, cam.blob, kModeNaive, hull, box);
    CHECK(hull.n == 0 || (hull.n >= 3 && hull.n <= 8), "hull of %d points", hull.n);
    if (round % 16 == 0) {  // the unit box is no box
        CullHull hull0;
        cull_hull_wh(W, H, cam.blob, kModeNaive, hull0);
        CHECK(!cull.boxed && memcmp(cr, cr0, sizeof cr) == 0 && hull.n == hull0.n, "the unit box: another rectangle or hull");
        for (int i = 0; i < hull.n && i < hull0.n; i++) CHECK(hull.x[i] == hull0.x[i] && hull.y[i] == hull0.y[i], "the unit box: hull point %d", i);
        CHECK(n_active == n_active0 && order == order0 && pos == pos0, "the unit box: another order");
    }
    for (uint32_t j = 0; j < ty; j++)
        for (uint32_t i = 0; i < tx; i++) {
            const uint32_t tile = j * tx + i;
            const bool inactive = tile_is_inactive(cull, (int64_t)i * ts, (int64_t)j * ts, ts);
            CHECK(inactive == (pos[tile] >= n_active), "tile %u: tile_is_inactive %d, position %u of %u active", tile, (int)inactive, pos[tile], n_active);
            for (int s = 0; s < 9; s++) {
                const uint32_t lx = s < 4 ? ((s & 1) ? ts - 1 : 0) : (s == 4 ? ts / 2 : pick(0, ts - 1));
                const uint32_t ly = s < 4 ? ((s & 2) ? ts - 1 : 0) : (s == 4 ? ts / 2 : pick(0, ts - 1));
                const uint32_t x = i * ts + lx, y = j * ts + ly;
                if (x >= W || y >= H) continue;
                const bool outside_rect = (int32_t)x < cr[0] || (int32_t)x >= cr[2] || (int32_t)y < cr[1] || (int32_t)y >= cr[3];
                if (!inactive && !outside_rect) continue;
                g_inactive_checked++;
                CHECK(!ray_hits(cam, box, W, H, x + 0.5, y + 0.5), "pixel (%u, %u) of %s hits the box (%ux%u ts %u, box %g %g %g - %g %g %g)", x, y,
                      inactive ? "an INACTIVE tile" : "outside the cull rectangle", W, H, ts, box.lo[0], box.lo[1], box.lo[2], box.hi[0], box.hi[1], box.hi[2]);
            }
        }
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 400;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!state) state = 1;
    for (int c = 0; c < cases; c++) fuzz_case(c);
    // the fuzz must have met what it is for
    CHECK(g_inactive_checked > 50L * cases, "only %ld culled pixels checked", g_inactive_checked);
    CHECK(g_fewer > cases / 4, "a box took tiles away in only %ld cases", g_fewer);
    CHECK(g_eye_in_box > cases / 40 && g_eye_in_cube > cases / 40 && g_no_cull > cases / 40, "eye in the box %ld, in the cube outside it %ld, cull disabled %ld", g_eye_in_box,
          g_eye_in_cube, g_no_cull);
    for (int k = 0; k < 6; k++) CHECK(g_kinds[k] > cases / 20, "camera kind %d drawn %d times", k, g_kinds[k]);
    if (g_bad) { printf("clip_hostmath_fuzz: %ld FAILURES\n", g_bad); return 1; }
    printf("clip_hostmath_fuzz: culled pixels %ld, fewer tiles in %ld cases, eye in box %ld / in cube %ld, no cull %ld\nclip_hostmath_fuzz: OK (%d cases)\n",
           g_inactive_checked, g_fewer, g_eye_in_box, g_eye_in_cube, g_no_cull, cases);
    return 0;
}
