// TEST INFRASTRUCTURE: the division-free block map of vokselis_amd/csrc/vk_hostmath.hpp -- udiv and the overloads of batch_block_split, deal_pos
// and tile_pixel that take the launch's reciprocals (BlockMapDesc), which is what the kernels run -- held to the '/'-based functions of the same
// header, which stay the definition.  Plain g++ with -fsanitize=address,undefined, run directly (a pool of threads over independent jobs, each seeded from the program's seed and its own number).  The reciprocals always come from
// block_map_make, the routine the launch calls (vk_render.hip: dispatch_march).
//
//   recip:   every divisor a launch constant can be -- n_frames 1..1024, tiles_x 1..260, ts / 8 and its square for ts in {8, 16, 24, 32, 40, 64, 72,
//            128, 1024}, the deal's k and k - 1 for k in 2..16 -- through a launch at the bound; udiv against n / d for the first 4 096 and the
//            last 4 096 numerators below 2^31 (2^31 - 1, the bound, among them) and 1 M seeded ones in between.
//   split:   batch_block_split for every ts x every n_frames in 1..1024 x both frame_runs.  A launch of one slot: every block index from 0 to the
//            padded grid size when that is at most 65 536, otherwise the first and last 4 096 and 1 M seeded ones; and the largest launch the
//            host accepts (just under 2^31 blocks): first and last 4 096 and 1 M seeded ones.
//   deal:    deal_pos for nranks 1..8 x root_skip in {0, 2..16, 17, 1000, 2^31 - 1, 2^31, 2^31 + 1, 2^32 - 1} (vk_partition_root_skip accepts everything
//            but 1) x every rank: every slot below 5 000; and at the largest launch the first and last 4 096 slots and 1 M seeded ones.
//   pixel:   tile_pixel for every ts x tiles_x 1..260: every tile id 0..3 tiles_x (the last stands for "no tile") at the first and last sub and
//            lane; every sub x every lane at two tiles; tile ids up to 2^31 - 1 (first and last 4 096, 1 M seeded) for every tiles_x.  The
//            output index as corner + lane part (compact_pixel_index of the corner, frame_block_base, block_lane_part) against
//            compact_pixel_index / frame_pixel_index of the pixel, origins off the screen included.
//   refuse:  block_map_make says no to a zero divisor, to 2^31 blocks and more, to 2^31 tiles and more, to a deal whose round could reach 2^31.
//
// Any mismatch fails.  The output states, per part, how many arguments were evaluated and what share of the part's argument space that is.
// usage: block_map_fuzz <seed>; prints "block_map_fuzz: OK ..." and exits 0, or the first failures and exits 1.
#include "vk_hostmath.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <thread>
#include <vector>

using namespace vk;

static thread_local uint64_t state;  // seeded per job
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static uint64_t below(uint64_t n) { return (uint64_t)(((unsigned __int128)rnd() * n) >> 64); }

static std::atomic<long> g_bad{0};
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (g_bad++ < 20) { printf("FAIL %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                 \
    } while (0)

static const uint32_t kTs[9] = {8, 16, 24, 32, 40, 64, 72, 128, 1024};
static const uint64_t kBound = kUDivBound;  // 2^31
static const uint64_t kMaxBlocks = (1ull << 31) - 513;  // the host's own limit: n_blocks < 2^31 - 512 (vk_render.hip, vk_batch.hip)

struct Tally { double evaluated = 0, space = 0; };
static void report(const char *name, const Tally &t) {
    printf("%-6s %.4g arguments evaluated of %.4g: %.5f %% of the argument space covered, %.5f %% left out by sampling\n", name, t.evaluated, t.space,
           100.0 * t.evaluated / t.space, 100.0 - 100.0 * t.evaluated / t.space);
}

// f(n) for the first and last `edge` values of [0, n_end) and `seeded` values in between (all of them when the range is small)
template <class F>
static void sweep(uint64_t n_end, uint64_t edge, uint64_t seeded, Tally &t, F f) {
    t.space += (double)n_end;
    if (n_end <= 2 * edge + seeded) { for (uint64_t n = 0; n < n_end; n++) f((uint32_t)n); t.evaluated += (double)n_end; return; }
    for (uint64_t n = 0; n < edge; n++) f((uint32_t)n);
    for (uint64_t n = n_end - edge; n < n_end; n++) f((uint32_t)n);
    for (uint64_t i = 0; i < seeded; i++) f((uint32_t)(edge + below(n_end - 2 * edge)));
    t.evaluated += (double)(2 * edge + seeded);
}

// the largest launch of (ts, n_frames, nranks, k) the host accepts, with its reciprocals
static uint64_t largest_launch(uint32_t ts, uint32_t tiles_x, uint32_t tiles_y, uint32_t n_frames, uint32_t nranks, uint32_t k, BlockMapDesc &m) {
    const uint64_t unit = (uint64_t)(ts / 8) * (ts / 8) * n_frames;
    uint64_t slots = kMaxBlocks / unit;
    if (nranks > 1 && k >= 2) slots = std::min(slots, (kBound - 1) * (k - 1) / k);  // round = slot + slot / (k - 1) stays below 2^31
    for (int tries = 0; tries < 4 && slots; tries++, slots--)
        if (block_map_make(ts, tiles_x, tiles_y, n_frames, nranks, k, slots * unit, m)) return slots * unit;
    CHECK(false, "no launch near the bound accepted: ts %u frames %u ranks %u k %u", ts, n_frames, nranks, k);
    return 0;
}

static void test_recip(Tally &t, uint32_t nf_lo, uint32_t nf_hi, bool rest) {
    auto one = [&](const char *what, uint32_t d, UDiv u) {
        sweep(kBound, 4096, 1000000, t, [&](uint32_t n) { CHECK(udiv(n, u) == n / d, "%s: %u / %u gives %u", what, n, d, udiv(n, u)); });
        CHECK(udiv((uint32_t)(kBound - 1), u) == (uint32_t)(kBound - 1) / d, "%s: the bound itself, d %u", what, d);
    };
    BlockMapDesc m;
    for (uint32_t nf = nf_lo; nf <= nf_hi; nf++) { if (largest_launch(8, 1, 1, nf, 1, 0, m)) one("n_frames", nf, m.n_frames); }
    if (!rest) return;
    for (uint32_t tx = 1; tx <= 260; tx++) { if (largest_launch(8, tx, 3, 1, 1, 0, m)) one("tiles_x", tx, m.tiles_x); }
    for (uint32_t ts : kTs) { if (largest_launch(ts, 1, 1, 1, 1, 0, m)) { one("per_tile", (ts / 8) * (ts / 8), m.per_tile); one("sps", ts / 8, m.sps); } }
    for (uint32_t k = 2; k <= 16; k++) { if (largest_launch(8, 1, 1, 1, 2, k, m)) { one("skip", k, m.skip); one("skip_m1", k - 1, m.skip_m1); } }
}

static void test_split(Tally &t, uint32_t ts, uint32_t nf_lo, uint32_t nf_hi) {
    auto same = [](uint32_t lb, uint32_t per_tile, uint32_t nf, bool runs, const BlockMapDesc &m) {
        const BlockSplit a = batch_block_split(lb, per_tile, nf, runs), b = batch_block_split(lb, per_tile, nf, runs, m);
        CHECK(a.slot == b.slot && a.frame == b.frame && a.sub == b.sub, "split: lb %u per_tile %u frames %u runs %d: (%u %u %u) against (%u %u %u)", lb, per_tile, nf,
              (int)runs, b.slot, b.frame, b.sub, a.slot, a.frame, a.sub);
    };
        for (uint32_t nf = nf_lo; nf <= nf_hi; nf++) {
            const uint32_t per_tile = (ts / 8) * (ts / 8);
            BlockMapDesc m;
            const uint64_t n_blocks = (uint64_t)per_tile * nf, grid = (n_blocks + 511) / 512 * 512;  // one slot
            CHECK(block_map_make(ts, 5, 3, nf, 1, 0, n_blocks, m), "a small launch refused: ts %u frames %u", ts, nf);
            BlockMapDesc M;
            const uint64_t big = largest_launch(ts, 5, 3, nf, 1, 0, M);
            for (int runs = 0; runs < 2; runs++) {
                if (grid <= 65536) sweep(grid, grid, 0, t, [&](uint32_t lb) { same(lb, per_tile, nf, runs != 0, m); });
                else sweep(grid, 4096, 1000000, t, [&](uint32_t lb) { same(lb, per_tile, nf, runs != 0, m); });
                if (big) sweep((big + 511) / 512 * 512, 4096, 1000000, t, [&](uint32_t lb) { same(lb, per_tile, nf, runs != 0, M); });
            }
        }
}

static void test_deal(Tally &t, uint32_t N) {
    std::vector<uint32_t> ks = {0u, 17u, 1000u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu};
    for (uint32_t k = 2; k <= 16; k++) ks.push_back(k);  // (1: vk_partition_root_skip refuses it)
        for (uint32_t k : ks) {
            const uint32_t kk = N > 1 ? k : 0u;  // what the host puts into the launch: one rank deals plainly
            BlockMapDesc m, M;
            CHECK(block_map_make(8, 5, 3, 1, N, kk, 5000, m), "a small launch refused: ranks %u k %u", N, kk);
            const uint64_t big = largest_launch(8, 5, 3, 1, N, kk, M);  // ts 8, one frame: a block is a slot
            for (uint32_t rank = 0; rank < N; rank++) {
                sweep(5000, 5000, 0, t, [&](uint32_t slot) { CHECK(deal_pos(rank, slot, N, kk) == deal_pos(rank, slot, N, kk, m), "deal: rank %u slot %u N %u k %u", rank, slot, N, kk); });
                if (big)
                    sweep(big, 4096, 1000000, t, [&](uint32_t slot) { CHECK(deal_pos(rank, slot, N, kk) == deal_pos(rank, slot, N, kk, M), "deal: rank %u slot %u N %u k %u", rank, slot, N, kk); });
                else t.space += (double)big;
            }
        }
}

static void test_pixel(Tally &t) {
    auto same = [](uint32_t ts, uint32_t tx, uint32_t tile, uint32_t sub, uint32_t lane, const BlockMapDesc &m) {
        const TilePixel a = tile_pixel(ts, tx, tile, sub, lane), b = tile_pixel(ts, tx, tile, sub, lane, m), c = tile_pixel(ts, tx, tile, sub, 0u, m);
        CHECK(a.lx == b.lx && a.ly == b.ly && a.rx == b.rx && a.ry == b.ry, "pixel: ts %u tiles_x %u tile %u sub %u lane %u", ts, tx, tile, sub, lane);
        // the kernel's form: the corner, and the lane's offsets on top
        CHECK(c.lx + (lane & 7u) == a.lx && c.ly + (lane >> 3) == a.ly && c.rx + (lane & 7u) == a.rx && c.ry + (lane >> 3) == a.ry, "corner: ts %u tiles_x %u tile %u sub %u lane %u", ts, tx, tile, sub, lane);
    };
    for (uint32_t ts : kTs) {
        const uint32_t per_tile = (ts / 8) * (ts / 8);
        for (uint32_t tx = 1; tx <= 260; tx++) {
            BlockMapDesc m;
            CHECK(block_map_make(ts, tx, 3, 1, 1, 0, (uint64_t)per_tile * 3 * tx, m), "a small launch refused: ts %u tiles_x %u", ts, tx);
            t.space += (double)(3 * tx + 1) * per_tile * 64;
            for (uint32_t tile = 0; tile <= 3 * tx; tile++)
                for (uint32_t sub : {0u, per_tile - 1u})
                    for (uint32_t lane : {0u, 63u}) { same(ts, tx, tile, sub, lane, m); t.evaluated += 1; }
            if (tx == 1 || tx == 7 || tx == 260)
                for (uint32_t tile : {0u, 3 * tx - 1u})
                    for (uint32_t sub = 0; sub < per_tile; sub++)
                        for (uint32_t lane = 0; lane < 64; lane++) { same(ts, tx, tile, sub, lane, m); t.evaluated += 1; }
            if (ts == 8) {  // tile ids up to the bound: as many rows as fit
                const uint32_t ty = (uint32_t)((kBound - 1) / tx);
                BlockMapDesc M;
                CHECK(block_map_make(ts, tx, ty, 1, 1, 0, 512, M), "a frame of %u x %u tiles refused", tx, ty);
                sweep((uint64_t)tx * ty + 1, 4096, 1000000, t, [&](uint32_t tile) { same(ts, tx, tile, 0, 63, M); });
            }
        }
    }
    // the output index: corner + lane part
    for (int i = 0; i < 200000; i++) {
        const uint32_t ts = kTs[below(9)], per_tile = (ts / 8) * (ts / 8), tx = 1 + (uint32_t)below(260), ty = 1 + (uint32_t)below(40), nf = 1 + (uint32_t)below(1024);
        const uint32_t W = (tx - 1) * ts + 1 + (uint32_t)below(ts), H = (ty - 1) * ts + 1 + (uint32_t)below(ts);
        const uint32_t tile = (uint32_t)below((uint64_t)tx * ty), sub = (uint32_t)below(per_tile), frame = (uint32_t)below(nf), slot = (uint32_t)below(4000);
        const int32_t ox = -(int32_t)below(3 * ts), oy = -(int32_t)below(3 * ts);  // a region origin at or off the screen's edge
        BlockMapDesc m;
        CHECK(block_map_make(ts, tx, ty, nf, 1, 0, (uint64_t)per_tile * nf * 4000, m) || (uint64_t)per_tile * nf * 4000 > kBound, "a launch refused: ts %u frames %u", ts, nf);
        const TilePixel c = tile_pixel(ts, tx, tile, sub, 0u, m);
        const int32_t x0 = ox + (int32_t)c.rx, y0 = oy + (int32_t)c.ry;
        const uint32_t rec = compact_record(slot, nf, frame);
        for (uint32_t lane = 0; lane < 64; lane++) {
            const TilePixel p = tile_pixel(ts, tx, tile, sub, lane);
            CHECK(compact_pixel_index(rec, ts, c.lx, c.ly) + block_lane_part(lane, ts) == compact_pixel_index(rec, ts, p.lx, p.ly), "compact index: ts %u sub %u lane %u", ts, sub, lane);
            const int32_t x = ox + (int32_t)p.rx, y = oy + (int32_t)p.ry;
            if (x < 0 || y < 0 || x >= (int32_t)W || y >= (int32_t)H) continue;  // never stored
            CHECK((size_t)(frame_block_base(frame, W, H, x0, y0) + (int64_t)block_lane_part(lane, W)) == frame_pixel_index(frame, W, H, (uint32_t)x, (uint32_t)y),
                  "frame index: frame %u W %u H %u corner (%d, %d) lane %u", frame, W, H, x0, y0, lane);
        }
    }
}

static void test_refuse() {
    BlockMapDesc m;
    CHECK(!block_map_make(0, 1, 1, 1, 1, 0, 1, m), "ts 0 accepted");
    CHECK(!block_map_make(12, 1, 1, 1, 1, 0, 1, m), "ts 12 accepted");
    CHECK(!block_map_make(8, 0, 1, 1, 1, 0, 1, m), "tiles_x 0 accepted");
    CHECK(!block_map_make(8, 1, 1, 0, 1, 0, 1, m), "n_frames 0 accepted");
    CHECK(!block_map_make(8, 1, 1, 1, 0, 0, 1, m), "nranks 0 accepted");
    CHECK(block_map_make(8, 1, 1, 1, 1, 0, kBound, m), "2^31 blocks (indices below 2^31) refused");
    CHECK(!block_map_make(8, 1, 1, 1, 1, 0, kBound + 1, m), "2^31 + 1 blocks accepted");
    CHECK(!block_map_make(8, 1u << 16, 1u << 15, 1, 1, 0, 512, m), "2^31 tiles accepted");
    CHECK(block_map_make(8, 65535, 32768, 1, 1, 0, 512, m), "just under 2^31 tiles refused");
    CHECK(!block_map_make(8, 1, 1, 1, 2, 2, 1ull << 30, m), "a deal whose round reaches 2^31 accepted");
    CHECK(block_map_make(8, 1, 1, 1, 2, 2, (1ull << 30) - 1, m), "a deal whose round stays below 2^31 refused");
    CHECK(block_map_make(8, 1, 1, 1, 1, 2, 1ull << 30, m), "one rank deals plainly: its root_skip refused a launch");
}

int main(int argc, char **argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 0) : 88172645463325252ull;
    test_refuse();
    // independent jobs, the long ones first; a job's random numbers depend on the seed and the job's number only, not on the thread that runs it
    struct Job { int part; std::function<void(Tally &)> run; Tally t; };
    std::vector<Job> jobs;
    jobs.push_back({3, [](Tally &t) { test_pixel(t); }, {}});
    for (uint32_t N = 8; N >= 1; N--) jobs.push_back({2, [N](Tally &t) { test_deal(t, N); }, {}});
    for (uint32_t lo = 1; lo <= 1024; lo += 64) jobs.push_back({0, [lo](Tally &t) { test_recip(t, lo, lo + 63, lo + 64 > 1024); }, {}});
    for (int i = 8; i >= 0; i--)
        for (uint32_t lo = 1; lo <= 1024; lo += 32) jobs.push_back({1, [i, lo](Tally &t) { test_split(t, kTs[i], lo, lo + 31); }, {}});
    std::atomic<size_t> next{0};
    const unsigned n_thr = std::min(16u, std::max(2u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < n_thr; i++)
        pool.emplace_back([&] {
            for (size_t j; (j = next++) < jobs.size();) { state = (seed ^ ((j + 1) * 0x9E3779B97F4A7C15ull)) | 1ull; jobs[j].run(jobs[j].t); }
        });
    for (auto &x : pool) x.join();
    Tally sum[4];
    for (auto &j : jobs) { sum[j.part].evaluated += j.t.evaluated; sum[j.part].space += j.t.space; }
    report("recip", sum[0]); report("split", sum[1]); report("deal", sum[2]); report("pixel", sum[3]);
    if (g_bad) { printf("block_map_fuzz: %ld FAILURES\n", g_bad.load()); return 1; }
    printf("block_map_fuzz: OK\n");
    return 0;
}
