// diff_fuzz.cpp -- vk_diff.hpp on the host, under ASan + UBSan: the library's own request validation in its order, q() at its clamps and
// on a NaN, the stopping predicate at equality, the automatic omega against a long double evaluation, one voxel's update against a double
// evaluation within one rounding per operation, and whole blocks of sweeps replayed on the host.  A stand-alone program:
//     diff_fuzz CASES SEED
// Per case a random volume, set, spacing, axis and omega: a block of sweeps through diff_update_voxel as the device runs it -- per
// colour the tiles in a shuffled order and a tile's voxels in a shuffled order, in place -- against the same block in raster order:
// bitwise the same state, delta and fluxes.
#include "vk_diff.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace vk;

static uint64_t g_state;
static uint64_t rnd() {  // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd_below(uint32_t n) { return (uint32_t)(rnd() % n); }
static float rnd_unit() { return (float)(rnd() >> 40) / 16777216.0f; }
template <class T>
static void shuffle(std::vector<T> &v) {
    for (size_t i = v.size(); i > 1; i--) std::swap(v[i - 1], v[rnd_below((uint32_t)i)]);
}

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static vk_diffusion_request plain() {
    vk_diffusion_request ok;
    std::memset(&ok, 0, sizeof ok);
    ok.lo = 0.3f; ok.hi = INFINITY; ok.spacing[0] = ok.spacing[1] = ok.spacing[2] = 1u; ok.check_every = 32u; ok.max_sweeps = 64u; ok.delta_tol = 1e-5f; ok.flux_tol = 1e-3f;
    return ok;
}

static void check_validation() {
    const vk_diffusion_request ok = plain();
    CHECK(diff_validate(&ok, true, false, false) == nullptr && diff_validate(&ok, false, true, false) == nullptr && diff_validate(&ok, false, false, true) == nullptr, "a plain request stands");
    CHECK(diff_validate(nullptr, true, true, true) != nullptr && std::strstr(diff_validate(nullptr, true, true, true), "NULL"), "NULL");
    // the order: every request below carries every later fault as well, and the first is the one reported
    struct Step { const char *word; void (*change)(vk_diffusion_request &); };
    const Step steps[] = {
        {"NaN", [](vk_diffusion_request &r) { r.hi = NAN; }},
        {"lo > hi", [](vk_diffusion_request &r) { r.lo = 1.0f; r.hi = 0.5f; }},
        {"axis must be", [](vk_diffusion_request &r) { r.axis = 3u; }},
        {"unknown flag", [](vk_diffusion_request &r) { r.flags = 4u; }},
        {"a spacing outside", [](vk_diffusion_request &r) { r.spacing[2] = 65u; }},
        {"omega must be", [](vk_diffusion_request &r) { r.omega = 2.0f; }},
        {"check_every outside", [](vk_diffusion_request &r) { r.check_every = 1025u; }},
        {"max_sweeps < check_every", [](vk_diffusion_request &r) { r.max_sweeps = 0u; }},
        {"delta_tol or flux_tol", [](vk_diffusion_request &r) { r.flux_tol = -1.0f; }},
        {"gain or fill_out", [](vk_diffusion_request &r) { r.fill_out = NAN; }},
    };
    const size_t n_steps = sizeof steps / sizeof steps[0];
    for (size_t first = 0; first < n_steps; first++) {
        vk_diffusion_request r = ok;
        for (size_t k = n_steps; k-- > first;) steps[k].change(r);
        if (first >= 7u && r.check_every > 1024u) r.check_every = 32u;  // (max_sweeps 0 is below any check_every that stands)
        const char *why = diff_validate(&r, false, false, false);
        CHECK(why && std::strstr(why, steps[first].word), "fault %zu: got \"%s\", expected \"%s\"", first, why ? why : "(accepted)", steps[first].word);
    }
    CHECK(std::strstr(diff_validate(&ok, false, false, false), "nowhere"), "no output");
    vk_diffusion_request r = ok;
    r.flags = VK_DIFF_INSTALL;
    CHECK(diff_validate(&r, false, false, false) == nullptr, "an install is an output");
    for (float w : {-0.0f, 1e-30f, 1.0f, 1.9999999f}) { r = ok; r.omega = w; CHECK(diff_validate(&r, true, false, false) == nullptr, "omega %g stands", (double)w); }
    for (float w : {-1e-30f, 2.0f, NAN, INFINITY, -INFINITY}) { r = ok; r.omega = w; CHECK(diff_validate(&r, true, false, false) != nullptr, "omega %g is refused", (double)w); }
    for (uint32_t k : {1u, 1024u}) { r = ok; r.check_every = k; r.max_sweeps = k; CHECK(diff_validate(&r, true, false, false) == nullptr, "check_every %u stands", k); }
    for (float t : {NAN, INFINITY, -1e-30f}) { r = ok; r.delta_tol = t; CHECK(diff_validate(&r, true, false, false) != nullptr, "delta_tol %g is refused", (double)t); }
    r = ok; r.delta_tol = 0.0f; r.flux_tol = 0.0f; r.gain = -3.0f; r.fill_out = -1.0f;
    CHECK(diff_validate(&r, true, false, false) == nullptr, "zero tolerances and negative finite gain and fill stand");
}

static void check_q_and_predicate() {
    CHECK(diff_q(0.0f) == 0 && diff_q(-0.0f) == 0 && diff_q(1.0f) == 1073741824ll && diff_q(-1.0f) == -1073741824ll, "unit");
    CHECK(diff_q(1048576.0f) == (1ll << 50) && diff_q(2e6f) == (1ll << 50) && diff_q(INFINITY) == (1ll << 50), "the upper clamp");
    CHECK(diff_q(-1048576.0f) == -(1ll << 50) && diff_q(-3e9f) == -(1ll << 50) && diff_q(-INFINITY) == -(1ll << 50), "the lower clamp");
    CHECK(diff_q(NAN) == -(1ll << 50), "a NaN takes the lower clamp");
    CHECK(diff_q(std::nextafterf(1048576.0f, 0.0f)) == (1ll << 50) - (1ll << 26), "the float below the clamp: exact");
    CHECK(diff_q(0.99f / 1073741824.0f) == 0 && diff_q(-0.99f / 1073741824.0f) == 0 && diff_q(1.5f / 1073741824.0f) == 1, "truncation towards zero");
    CHECK(diff_flux_in_q(0.75f) == (1ll << 29) && diff_flux_out_q(0.75f) == 3ll << 29, "the faces' terms");
    for (int k = 0; k < 2000; k++) {
        const float t = (rnd_unit() - 0.5f) * 4.0f;
        const long double exact = (long double)t * 1073741824.0L;
        CHECK(diff_q(t) == (int64_t)exact, "q(%a)", (double)t);
    }
    // the predicate at equality, and one unit off
    CHECK(diff_converged(1e-5f, 1000, 1000, 1e-5f, 0.0f) && !diff_converged(std::nextafterf(1e-5f, 1.0f), 1000, 1000, 1e-5f, 1.0f), "delta at its bound");
    CHECK(diff_converged(0.0f, 1001000, 999000, 0.0f, 0.002f) == ((double)2000 <= (double)0.002f * 1000000.0), "the gap at its bound, as the doubles say");
    CHECK(diff_converged(0.0f, 1024, 1024 - 256, 0.0f, 0.25f + 0.03125f) == (256.0 <= (double)(0.25f + 0.03125f) * 896.0) && !diff_converged(0.0f, 1024, 768, 0.0f, 0.25f), "exact binary bounds");
    CHECK(diff_converged(0.0f, 7, 7, 0.0f, 0.0f) && diff_converged(0.0f, 0, 0, 0.0f, 0.0f) && !diff_converged(0.0f, 1, 0, 0.0f, 1.0f), "zero fluxes");
    CHECK(!diff_converged(0.0f, -5, 5, 0.0f, 1.0f) && !diff_converged(0.0f, -5, -5, 0.0f, 1.0f), "negative fluxes: the mean is what it is, and nothing is below it");
}

static void check_omega() {
    for (uint32_t n : {0u, 1u, 2u, 11u, 70u, 255u, 512u, 100000u, 50000000u}) {
        const long double exact = 2.0L / (1.0L + 3.141592653589793L / ((long double)n + 1.0L));
        const float got = diff_auto_omega(n);
        CHECK(got > 0.0f && got < 2.0f, "omega(%u) = %g lies in (0, 2)", n, (double)got);
        CHECK(std::fabs((long double)got - exact) <= 1.3e-7L * 2.0L, "omega(%u) = %.9g, exact %.9Lg", n, (double)got, exact);
        CHECK(got == (float)(2.0 / (1.0 + 3.141592653589793 / (double)((uint64_t)n + 1u))), "omega(%u): the header's expression", n);
    }
    CHECK(diff_auto_omega(0xffffffffu) == std::nextafterf(2.0f, 0.0f) && diff_auto_omega(400000000u) < 2.0f, "an extent whose omega would round to 2 takes the float below");
    vk_diffusion_request r = plain();
    CHECK(diff_omega(&r, 11u) == diff_auto_omega(11u), "0 asks for the automatic one");
    r.omega = 1.25f;
    CHECK(diff_omega(&r, 11u) == 1.25f, "a given omega is used");
    const uint32_t sp[3] = {1u, 2u, 64u};
    const DiffWeights W = diff_weights(sp, 1u);
    CHECK(W.w[0] == 1.0f && W.w[1] == 0.25f && W.w[2] == 1.0f / 4096.0f && W.g == 0.5f, "weights");
    const uint32_t sp3[3] = {3u, 1u, 1u};
    CHECK(diff_weights(sp3, 0u).w[0] == (float)(1.0 / 9.0) && diff_weights(sp3, 0u).g == 2.0f * (float)(1.0 / 9.0), "weights of a pitch of 3");
}

struct HostLoad { static uint32_t load(const uint32_t *p, uint32_t i) { return p[i]; } };

static void check_update_against_double() {
    for (int k = 0; k < 4000; k++) {
        uint32_t a[27];
        const uint32_t sp[3] = {1u + rnd_below(4u), 1u + rnd_below(4u), 1u + rnd_below(4u)};
        const uint32_t axis = rnd_below(3u);
        const DiffWeights W = diff_weights(sp, axis);
        for (uint32_t &w : a) w = rnd_below(4u) ? diff_bits(rnd_unit()) : kDiffOff;
        const bool inlet = rnd_below(4u) == 0u, outlet = rnd_below(4u) == 0u;
        const float omega = 0.1f + 1.85f * rnd_unit(), c = rnd_unit();
        a[13] = diff_bits(c);
        float got = -1.0f;
        const bool upd = diff_update_voxel<HostLoad>((const uint32_t *)a, 1u, 1u, 1u, 3u, 3u, 3u, W, inlet, outlet, omega, c, got);
        const uint32_t at[6] = {12u, 14u, 10u, 16u, 4u, 22u};
        double num = 0.0, den = 0.0;
        int terms = 0;
        for (int j = 0; j < 6; j++)
            if (a[at[j]] != kDiffOff) { num += (double)W.w[j >> 1] * (double)diff_float(a[at[j]]); den += (double)W.w[j >> 1]; terms++; }
        if (inlet) { num += (double)W.g; den += (double)W.g; terms++; }
        if (outlet) { den += (double)W.g; terms++; }
        CHECK(upd == (den != 0.0), "updated iff den != 0");
        if (!upd) { CHECK(got == -1.0f, "no update leaves the output alone"); continue; }
        const double gs = num / den, want = (double)c + (double)omega * (gs - (double)c);
        // one rounding per operation: at most 2 * terms + 4 of them, on values of magnitude at most num, den, 1 and 2
        const double eps = 5.97e-8, bound = eps * ((2.0 * terms + 1.0) * (num / den + 1.0) + 4.0) * (1.0 + (double)omega);
        CHECK(std::fabs((double)got - want) <= bound, "update %g, in double %g, bound %g", (double)got, want, bound);
    }
    // an edge voxel of the array: the neighbours outside do not exist
    uint32_t line[3] = {diff_bits(0.25f), diff_bits(0.5f), diff_bits(1.0f)};
    const uint32_t one[3] = {1u, 1u, 1u};
    const DiffWeights W = diff_weights(one, 0u);
    float got = 0.0f;
    CHECK(diff_update_voxel<HostLoad>((const uint32_t *)line, 0u, 0u, 0u, 3u, 1u, 1u, W, true, false, 1.0f, 0.25f, got) && got == (0.5f + 2.0f) / 3.0f, "the inlet end of a line: %g", (double)got);
    CHECK(diff_update_voxel<HostLoad>((const uint32_t *)line, 2u, 0u, 0u, 3u, 1u, 1u, W, false, true, 1.0f, 1.0f, got) && got == 1.0f + (0.5f / 3.0f - 1.0f), "the outlet end of a line: %g", (double)got);
    uint32_t lone[1] = {diff_bits(0.5f)};
    CHECK(!diff_update_voxel<HostLoad>((const uint32_t *)lone, 0u, 0u, 0u, 1u, 1u, 1u, W, false, false, 1.0f, 0.5f, got), "a lone voxel: den == 0");
    CHECK(diff_update_voxel<HostLoad>((const uint32_t *)lone, 0u, 0u, 0u, 1u, 1u, 1u, W, true, true, 1.0f, 0.5f, got) && got == 0.5f, "a voxel on both faces settles at one half: %g", (double)got);
}

struct Block { std::vector<uint32_t> state; uint32_t delta_bits; int64_t fin, fout; };

// one block of `sweeps` sweeps; order: nullptr for raster order, else per colour the voxels of that colour in the order to take
static Block run_block(std::vector<uint32_t> state, uint32_t nx, uint32_t ny, uint32_t nz, const DiffWeights &W, uint32_t axis, uint32_t first, uint32_t last, float omega, uint32_t sweeps,
                       bool shuffled) {
    Block b;
    b.delta_bits = 0u;
    const uint32_t ntx = (nx + kLabelTile.tx - 1u) / kLabelTile.tx, nty = (ny + kLabelTile.ty - 1u) / kLabelTile.ty, ntz = (nz + kLabelTile.tz - 1u) / kLabelTile.tz;
    for (uint32_t s = 0; s < sweeps; s++)
        for (uint32_t colour = 0; colour < 2u; colour++) {
            std::vector<uint32_t> tiles(ntx * nty * ntz);
            for (uint32_t t = 0; t < tiles.size(); t++) tiles[t] = t;
            if (shuffled) shuffle(tiles);
            for (uint32_t t : tiles) {
                uint32_t tx, ty, tz;
                tile_coords(t, ntx, nty, tx, ty, tz);
                std::vector<uint32_t> cells(kLabelTileVoxels);
                for (uint32_t e = 0; e < kLabelTileVoxels; e++) cells[e] = e;
                if (shuffled) shuffle(cells);
                for (uint32_t e : cells) {
                    uint32_t lx, ly, lz;
                    label_local_coords(e, lx, ly, lz);
                    const uint32_t x = tx * kLabelTile.tx + lx, y = ty * kLabelTile.ty + ly, z = tz * kLabelTile.tz + lz;
                    if (x >= nx || y >= ny || z >= nz || ((x + y + z) & 1u) != colour) continue;
                    const size_t i = (size_t)voxel_index(x, y, z, nx, ny);
                    if (state[i] == kDiffOff) continue;
                    const uint32_t p[3] = {x, y, z};
                    const float c = diff_float(state[i]);
                    float next = 0.0f;
                    if (!diff_update_voxel<HostLoad>((const uint32_t *)state.data(), x, y, z, nx, ny, nz, W, p[axis] == first, p[axis] == last, omega, c, next)) continue;
                    if (s + 1u == sweeps) { const float moved = next - c; b.delta_bits = std::max(b.delta_bits, diff_bits(std::fabs(moved))); }
                    state[i] = diff_bits(next);
                }
            }
        }
    uint64_t fin = 0, fout = 0;
    for (uint32_t z = 0; z < nz; z++)
        for (uint32_t y = 0; y < ny; y++)
            for (uint32_t x = 0; x < nx; x++) {
                const uint32_t w = state[(size_t)voxel_index(x, y, z, nx, ny)], p[3] = {x, y, z};
                if (w == kDiffOff) continue;
                if (p[axis] == first) fin += (uint64_t)diff_flux_in_q(diff_float(w));
                if (p[axis] == last) fout += (uint64_t)diff_flux_out_q(diff_float(w));
            }
    b.fin = (int64_t)fin; b.fout = (int64_t)fout;
    b.state = std::move(state);
    return b;
}

static void check_replayed_blocks(int n_cases) {
    for (int k = 0; k < n_cases; k++) {
        const uint32_t nx = 1u + rnd_below(40u), ny = 1u + rnd_below(20u), nz = 1u + rnd_below(11u);
        const uint32_t sp[3] = {1u + rnd_below(3u), 1u + rnd_below(3u), 1u + rnd_below(3u)};
        const uint32_t axis = rnd_below(3u), dims[3] = {nx, ny, nz};
        const DiffWeights W = diff_weights(sp, axis);
        const float omega = rnd_below(3u) ? diff_auto_omega(dims[axis]) : 0.2f + 1.75f * rnd_unit();
        const uint32_t density = 1u + rnd_below(10u);
        std::vector<uint32_t> state((size_t)nx * ny * nz);
        for (uint32_t &w : state) w = rnd_below(10u) < density ? diff_bits(0.5f) : kDiffOff;
        const uint32_t sweeps = 1u + rnd_below(6u);
        Block a = run_block(state, nx, ny, nz, W, axis, 0u, dims[axis] - 1u, omega, sweeps, false), b = run_block(state, nx, ny, nz, W, axis, 0u, dims[axis] - 1u, omega, sweeps, true);
        CHECK(a.state == b.state && a.delta_bits == b.delta_bits && a.fin == b.fin && a.fout == b.fout, "case %d (%u x %u x %u, %u sweeps): a shuffled order changes the block", k, nx, ny, nz,
              sweeps);
        for (size_t i = 0; i < state.size(); i++) {
            CHECK((state[i] == kDiffOff) == (a.state[i] == kDiffOff), "the set is what it was");
            if (a.state[i] != kDiffOff) CHECK(std::isfinite(diff_float(a.state[i])), "a finite value on the set");
        }
        // a second block from the first one's state, again both ways
        Block a2 = run_block(a.state, nx, ny, nz, W, axis, 0u, dims[axis] - 1u, omega, 2u, false), b2 = run_block(b.state, nx, ny, nz, W, axis, 0u, dims[axis] - 1u, omega, 2u, true);
        CHECK(a2.state == b2.state && a2.delta_bits == b2.delta_bits && a2.fin == b2.fin && a2.fout == b2.fout, "case %d: the second block", k);
    }
}

int main(int argc, char **argv) {
    const int n_cases = argc > 1 ? std::atoi(argv[1]) : 100;
    g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!g_state) g_state = 1;
    check_validation();
    check_q_and_predicate();
    check_omega();
    check_update_against_double();
    check_replayed_blocks(n_cases);
    std::printf("OK (%d cases)\n", n_cases);
    return 0;
}
