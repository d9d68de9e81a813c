// dist_fuzz.cpp -- vk_dist.hpp on the host, under ASan + UBSan: the library's own line function, column arithmetic, overflow bound and
// request validation.  A stand-alone program:
//     dist_fuzz CASES SEED
// Per case a random line -- runs of INF, all INF, a single entry, length 1, heights up to the largest the bound allows, spacing 1 .. 64,
// a stride above 1 -- through dist_line against the minimum over all pairs, with both scans' trips held to 2 n and n and every array
// exactly as long as the line needs (ASan sees the rest); and a small random volume through the three passes as the kernels compose
// them against the distance by its definition.
#include "vk_dist.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace vk;

static uint64_t g_state;
static uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

// out(i) by the definition: the minimum over all j
static uint32_t quadratic(const std::vector<uint32_t> &g, const std::vector<uint32_t> &finite, uint32_t i, uint32_t w) {
    uint64_t best = std::numeric_limits<uint64_t>::max();
    for (uint32_t j : finite) {
        const uint64_t off = (uint64_t)w * (i > j ? i - j : j - i);
        if (g[j] + off * off < best) best = g[j] + off * off;
    }
    return best == std::numeric_limits<uint64_t>::max() ? kDistInf : (uint32_t)best;
}

static void check_line(const std::vector<uint32_t> &g, uint32_t w, uint32_t stride, const char *what) {
    const uint32_t n = (uint32_t)g.size();
    const uint64_t base = rnd_below(stride), len = base + (uint64_t)(n - 1u) * stride + 1u;  // exactly as long as the last entry needs
    std::vector<uint32_t> gs(len, 0x5a5a5a5au), stack(len, 0u), out(len, 0x77777777u);
    for (uint32_t k = 0; k < n; k++) gs[base + (uint64_t)k * stride] = g[k];
    const DistTrips t = dist_line(gs.data(), stack.data(), out.data(), base, stride, n, w);
    CHECK(t.build <= 2u * n && t.read == n, "%s: n %u w %u: %u build trips, %u read trips", what, n, w, t.build, t.read);
    std::vector<uint32_t> finite;  // the entries that carry a parabola
    for (uint32_t j = 0; j < n; j++)
        if (g[j] != kDistInf) finite.push_back(j);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t want = quadratic(g, finite, i, w), got = out[base + (uint64_t)i * stride];
        CHECK(got == want, "%s: n %u w %u stride %u: out[%u] = %u, the minimum over all pairs is %u", what, n, w, stride, i, got, want);
    }
    for (uint64_t k = 0; k < len; k++)
        if (k < base || (k - base) % stride) CHECK(out[k] == 0x77777777u && stack[k] == 0u, "%s: entry %llu between the line's entries was written", what, (unsigned long long)k);
}

static void fuzz_line() {
    const uint32_t w = rnd_below(8) == 0 ? (rnd_below(2) ? 1u : (uint32_t)VK_DIST_MAX_SPACING) : 1u + rnd_below(VK_DIST_MAX_SPACING);
    const uint32_t most = 0xffffu / w + 1u;  // w (n - 1) <= 0xffff
    uint32_t n = 1u + rnd_below(most < 400u ? most : 400u);
    if (rnd_below(10) == 0) n = 1u;
    if (rnd_below(40) == 0 && most <= 4096u) n = most;  // the longest line this spacing allows (spacing 1 .. 15: the fixed corners in main)
    const uint64_t reach = (uint64_t)w * (n - 1u) * w * (n - 1u);
    const uint32_t top = (uint32_t)(kDistMaxD2 - reach);  // the largest height whose parabola stays finite over the whole line
    std::vector<uint32_t> g(n);
    const uint32_t mode = rnd_below(8);
    for (uint32_t k = 0; k < n; k++) {
        switch (mode) {
            case 0: g[k] = kDistInf; break;                                                         // no parabola at all
            case 1: g[k] = rnd_below(3) ? 0u : kDistInf; break;                                     // a set's own indicator
            case 2: g[k] = rnd_below(4) ? kDistInf : top - rnd_below(top < 1000u ? top + 1u : 1000u); break;  // heights near 2^32
            case 3: g[k] = (uint32_t)(rnd() % ((uint64_t)top + 1u)); break;                         // anything
            case 4: g[k] = (k / (1u + n / 7u)) % 2u ? kDistInf : rnd_below(50); break;              // runs of INF
            case 5: g[k] = (w * rnd_below(6)) * (w * rnd_below(6)); break;                          // what a column pass leaves: small squares, many ties
            case 6: g[k] = kDistInf; break;                                                         // (a single entry: below)
            default: g[k] = rnd_below(2) ? top : 0u; break;                                         // the two extremes side by side
        }
    }
    if (mode == 6) g[rnd_below(n)] = rnd_below(2) ? 0u : top;
    check_line(g, w, rnd_below(3) ? 1u : 2u + rnd_below(5), "line");
}

// a small volume through the column pass and the two line passes, as the kernels run them, against the definition
static void fuzz_volume() {
    const uint32_t nx = 1u + rnd_below(9), ny = 1u + rnd_below(9), nz = 1u + rnd_below(9);
    const uint32_t w[3] = {1u + rnd_below(VK_DIST_MAX_SPACING), 1u + rnd_below(VK_DIST_MAX_SPACING), 1u + rnd_below(VK_DIST_MAX_SPACING)};
    uint64_t bound = 0;
    CHECK(dist_d2_fits(w, nx, ny, nz, &bound) && bound <= kDistMaxD2, "a volume of %u x %u x %u at spacing 64 at most fits", nx, ny, nz);
    const uint64_t n = (uint64_t)nx * ny * nz, slice = (uint64_t)nx * ny;
    const uint32_t density = rnd_below(5);
    std::vector<uint8_t> target(n);
    for (auto &t : target) t = density == 0 ? 0u : (density == 4 ? 1u : rnd_below(4) < density);
    std::vector<uint32_t> a(n), b(n), stack(n);
    for (uint64_t col = 0; col < slice; col++) {
        uint32_t steps = kDistInf;
        for (uint32_t z = 0; z < nz; z++) { steps = dist_step_advance(steps, target[col + z * slice] != 0u); a[col + z * slice] = steps; }
        uint32_t back = kDistInf;
        for (uint32_t z = nz; z-- > 0u;) {
            const uint32_t below = a[col + z * slice];
            back = dist_step_advance(back, below == 0u);
            a[col + z * slice] = dist_steps_squared(below < back ? below : back, w[2]);
        }
    }
    for (uint64_t line = 0; line < (uint64_t)nx * nz; line++) (void)dist_line(a.data(), stack.data(), b.data(), line % nx + line / nx * slice, nx, ny, w[1]);
    for (uint64_t line = 0; line < (uint64_t)ny * nz; line++) (void)dist_line(b.data(), stack.data(), a.data(), line * nx, 1u, nx, w[0]);
    for (uint64_t v = 0; v < n; v++) {
        uint64_t best = std::numeric_limits<uint64_t>::max();
        const int64_t vx = (int64_t)(v % nx), vy = (int64_t)(v / nx % ny), vz = (int64_t)(v / slice);
        for (uint64_t u = 0; u < n; u++) {
            if (!target[u]) continue;
            const int64_t dx = w[0] * (vx - (int64_t)(u % nx)), dy = w[1] * (vy - (int64_t)(u / nx % ny)), dz = w[2] * (vz - (int64_t)(u / slice));
            const uint64_t d = (uint64_t)(dx * dx + dy * dy + dz * dz);
            if (d < best) best = d;
        }
        const uint32_t want = best == std::numeric_limits<uint64_t>::max() ? kDistInf : (uint32_t)best;
        CHECK(a[v] == want, "volume %u x %u x %u: D2 at %llu is %u, by the definition %u", nx, ny, nz, (unsigned long long)v, a[v], want);
    }
}

static void check_validation() {
    vk_distance_request ok{};
    ok.lo = 0.3f; ok.hi = INFINITY; ok.op = VK_DIST_OUTSIDE; ok.spacing[0] = ok.spacing[1] = ok.spacing[2] = 1u;
    CHECK(dist_validate(&ok, true, false, false) == nullptr && dist_validate(&ok, false, false, true) == nullptr, "a plain distance request stands");
    CHECK(dist_validate(nullptr, true, false, false) != nullptr, "NULL");
    CHECK(dist_validate(&ok, false, false, false) != nullptr, "nothing requested");
    CHECK(dist_validate(&ok, true, true, false) != nullptr, "dense_out with a distance op");
    auto bad = [&](auto &&change, bool d2 = true, bool dense = false, bool result = false) {
        vk_distance_request r = ok;
        change(r);
        return dist_validate(&r, d2, dense, result) != nullptr;
    };
    CHECK(bad([](vk_distance_request &r) { r.lo = NAN; }) && bad([](vk_distance_request &r) { r.hi = NAN; }) && bad([](vk_distance_request &r) { r.lo = 1.0f; r.hi = 0.5f; }), "range");
    CHECK(bad([](vk_distance_request &r) { r.op = 6; }) && bad([](vk_distance_request &r) { r.op = -1; }) && bad([](vk_distance_request &r) { r.flags = 4u; }), "op, flag");
    for (int c = 0; c < 3; c++)
        CHECK(bad([c](vk_distance_request &r) { r.spacing[c] = 0u; }) && bad([c](vk_distance_request &r) { r.spacing[c] = 65u; }) && !bad([c](vk_distance_request &r) { r.spacing[c] = 64u; }), "spacing");
    CHECK(bad([](vk_distance_request &r) { r.radius = 1.0f; }) && bad([](vk_distance_request &r) { r.flags = VK_DIST_INSTALL; }), "a radius, INSTALL with a distance op");
    CHECK(bad([](vk_distance_request &r) { r.fill_in = INFINITY; }) && bad([](vk_distance_request &r) { r.fill_out = NAN; }), "fills");
    for (int op = VK_DIST_DILATE; op <= VK_DIST_OPEN; op++) {
        auto morph = [op](vk_distance_request &r) { r.op = op; r.radius = 1.5f; };
        CHECK(!bad(morph, false, true) && !bad(morph, false, false, true) && bad(morph, true, true) && bad(morph, false, false, false), "op %d: outputs", op);
        CHECK(!bad([op](vk_distance_request &r) { r.op = op; r.flags = VK_DIST_INSTALL | VK_DIST_CLIP_BOX; }, false), "op %d: INSTALL alone is a request", op);
        CHECK(bad([op](vk_distance_request &r) { r.op = op; r.radius = -1.0f; }, false, true) && bad([op](vk_distance_request &r) { r.op = op; r.radius = INFINITY; }, false, true) &&
              bad([op](vk_distance_request &r) { r.op = op; r.radius = NAN; }, false, true) && bad([op](vk_distance_request &r) { r.op = op; r.radius = 65536.0f; }, false, true) &&
              !bad([op](vk_distance_request &r) { r.op = op; r.radius = 65535.0f; }, false, true) && !bad([op](vk_distance_request &r) { r.op = op; r.radius = 0.0f; }, false, true), "op %d: radius", op);
    }
    CHECK(dist_r2(1.5f) == 2u && dist_r2(3.3f) == 10u && dist_r2(0.0f) == 0u && dist_r2(65535.0f) == 4294836225ull && dist_r2(65535.0f) < kDistInf, "R2");
    // the overflow bound, at its edge on every axis: 64 * 1023 = 65472 fits, 64 * 1024 does not; and the sum of three
    const uint32_t w64[3] = {64u, 64u, 64u}, w1[3] = {1u, 1u, 1u};
    CHECK(dist_d2_fits(w64, 1024u, 1u, 1u) && !dist_d2_fits(w64, 1025u, 1u, 1u) && dist_d2_fits(w64, 1u, 1024u, 1u) && !dist_d2_fits(w64, 1u, 1u, 1025u), "one axis");
    CHECK(dist_d2_fits(w1, 65536u, 1u, 1u) && !dist_d2_fits(w1, 65537u, 1u, 1u) && !dist_d2_fits(w1, 0xffffffffu, 1u, 1u), "spacing 1");
    CHECK(dist_d2_fits(w1, 37838u, 37838u, 37838u) && !dist_d2_fits(w1, 37839u, 37838u, 37838u), "three axes: 3 * 37837^2 = 4294915707, and 37838^2 more does not fit");
    uint64_t bound = 0;
    CHECK(dist_d2_fits(w64, 900u, 1u, 1u, &bound) && bound == 3310391296ull && bound > (1ull << 31), "the bound of the longest test volume");
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 300;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!g_state) g_state = 1;
    check_validation();
    // the fixed corners: length 1, all INF, a single entry at either end, the largest heights on the longest line
    check_line({kDistInf}, 1u, 1u, "length 1, INF");
    check_line({0u}, 64u, 3u, "length 1");
    check_line({kDistInf, kDistInf, kDistInf}, 7u, 1u, "all INF");
    for (uint32_t w : {1u, 64u}) {
        const uint32_t n = 0xffffu / w + 1u;
        std::vector<uint32_t> g(n, kDistInf);
        g[0] = (uint32_t)(kDistMaxD2 - (uint64_t)w * (n - 1u) * w * (n - 1u));
        check_line(g, w, 1u, "the longest line, one entry at its start");
        g[0] = kDistInf; g[n - 1u] = 0u;
        check_line(g, w, 1u, "the longest line, one entry at its end");
    }
    for (int k = 0; k < cases; k++) {
        fuzz_line();
        if (k % 4 == 0) fuzz_volume();
    }
    std::printf("OK (%d cases)\n", cases);
    return 0;
}
