// vk_hostmath.hpp -- the index arithmetic that decides which pixel lands where: the deal of tile positions over ranks, the block -> pixel
// map of a launch, the compact (slot, frame) records of a partition, the root's un-tile map, and the host-side geometry of a frame (cull
// rectangle, silhouette hull, heaviest-first tile order; the reference's tile loop is examples/xor/main.rs:77-95,235-254).
//
// No HIP in here: the kernels (vk_common.hpp, vk_post.hpp) and the host (vk_order.hip, vk_batch.hip) include it, and so does
// tests/hostmath_fuzz.cpp, a plain g++ -fsanitize=address,undefined program that replays a whole partition -> gather -> un-tile on the CPU
// with these very functions (tile sizes 8..1024, frame shapes that are not multiples of the tile, 1..8 ranks, weighted deals, 1..64 frames).
// The kernels run the block map without a division (UDiv, block_map_make and the overloads that take a BlockMapDesc, below);
// tests/block_map_fuzz.cpp holds those to the '/'-based functions here, which stay the definition.
#pragma once

#include <stdint.h>
#include <stddef.h>

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define VK_HD __host__ __device__ __forceinline__
#else
#define VK_HD inline
#endif

namespace vk {

// ---- dealing positions of the heaviest-first order to ranks ------------------------------------
// Round j gives one position to every rank, in rank order.  With root_skip = k >= 2 the root (rank 0) sits out every
// k-th round (rounds k-1, 2k-1, ...): it also un-tiles every frame, and a lighter share of the march keeps it from
// being the rank everybody waits for.  k < 2: plain round robin, position q -> rank q % N, slot q / N.
VK_HD uint32_t deal_pos(uint32_t rank, uint32_t slot, uint32_t N, uint32_t k) {
    if (k < 2u) return rank + slot * N;
    const uint32_t round = rank ? slot : slot + slot / (k - 1u);  // the root's slot j is its j-th full round
    const uint32_t start = round * N - round / k;                 // one position less for every light round before
    return start + rank - ((round % k) == k - 1u ? 1u : 0u);      // (the root never sees a light round)
}
VK_HD void deal_owner(uint32_t pos, uint32_t N, uint32_t k, uint32_t &rank, uint32_t &slot) {
    if (k < 2u) { rank = pos % N; slot = pos / N; return; }
    const uint32_t G = k * N - 1u, g = pos / G, o = pos - g * G;  // a group: k - 1 full rounds and a light one
    uint32_t rj;
    if (o < (k - 1u) * N) { rj = o / N; rank = o - rj * N; }
    else { rj = k - 1u; rank = o - (k - 1u) * N + 1u; }
    slot = rank ? g * k + rj : g * (k - 1u) + rj;
}
// rounds needed to deal `tiles` positions = slots of a non-root rank
VK_HD uint32_t deal_rounds(uint32_t tiles, uint32_t N, uint32_t k) {
    if (k < 2u) return (tiles + N - 1u) / N;
    uint32_t r = tiles / N;
    while (r * N - r / k < tiles) r++;
    return r;
}

// ---- physical workgroup -> logical 8x8 block ---------------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an XCD's L2).  A group of 512 consecutive physical
// blocks is mapped so that each XCD receives 64 consecutive logical blocks = the 64 waves of one 64x64 pixel tile: neighbouring
// rays share an L2, while successive tiles still spread over all XCDs.  A bijection on every multiple of 512 (grids are padded to one).
VK_HD uint32_t logical_block(uint32_t b) {
    const uint32_t group = b >> 9, r = b & 511u;
    return (group << 9) + ((r & 7u) << 6) + (r >> 3);
}
// The staged march's 256-thread groups: workgroup G (round-robin over the XCDs: a run of 128 consecutive groups gives every XCD the 16
// groups of one 64 x 64 tile) and its wave -> the logical 8x8 block; the four waves of a group are the 2 x 2 neighbouring blocks of a tile
// (tile edge a multiple of 16).  A bijection between (G, wave) and the blocks of whole runs of 128 groups.
VK_HD uint32_t group_logical_block(uint32_t G, uint32_t wave, uint32_t ts) {
    const uint32_t chunk = G >> 7, rr = G & 127u;
    const uint32_t LG = (chunk << 7) + ((rr & 7u) << 4) + (rr >> 3);
    const uint32_t sps = ts >> 3, per_tile = sps * sps, hq = sps >> 1;  // 8x8 blocks per tile edge (even), quads per tile edge
    const uint32_t l4 = LG * 4u + wave, u = l4 % per_tile, q = u >> 2, w = u & 3u;
    const uint32_t qy = q / hq, qx = q - qy * hq;
    return (l4 - u) + (2u * qy + (w >> 1)) * sps + 2u * qx + (w & 1u);
}

// ---- a launch's logical block -> (slot, frame, 8x8 block inside the tile) -------------------------
// Batched launches are position-major: (slot, frame) pairs with the frame running fastest, per_tile blocks each.  With
// frame_runs the frame index is relabelled so that the 8 consecutive pairs the launch hands to the 8 XCDs are runs of
// CONSECUTIVE frames of one tile position instead of frames x, x + 8, ... (vk_common.hpp: frame_view).
struct BlockSplit { uint32_t slot, frame, sub; };
VK_HD BlockSplit batch_block_split(uint32_t lb, uint32_t per_tile, uint32_t n_frames, bool frame_runs) {
    BlockSplit s;
    const uint32_t g = lb / per_tile;
    s.sub = lb - g * per_tile;
    s.slot = g / n_frames;
    uint32_t fr = g - s.slot * n_frames;
    if (frame_runs) {
        const uint32_t x = fr & 7u, j = fr >> 3, q = n_frames >> 3, rem = n_frames & 7u;
        fr = x * q + (x < rem ? x : rem) + j;
    }
    s.frame = fr;
    return s;
}

// The pixel a lane of an 8x8 block holds: (lx, ly) inside its tile, (rx, ry) inside the launch's region.
struct TilePixel { uint32_t lx, ly, rx, ry; };
VK_HD TilePixel tile_pixel(uint32_t ts, uint32_t tiles_x, uint32_t tile, uint32_t sub, uint32_t lane) {
    TilePixel p;
    const uint32_t sps = ts >> 3;  // 8x8 blocks per tile edge
    const uint32_t tty = tile / tiles_x, ttx = tile - tty * tiles_x;
    const uint32_t sy = sub / sps, sx = sub - sy * sps;
    p.lx = sx * 8u + (lane & 7u); p.ly = sy * 8u + (lane >> 3);
    p.rx = ttx * ts + p.lx; p.ry = tty * ts + p.ly;
    return p;
}
// ---- the same map without a division: what the kernels run (vk_common.hpp: frame_view, map_pixel) -------------------------------
// Every divisor of the map above is a constant of the launch, so the host hands the kernel a reciprocal for each (LaunchDesc::bm)
// and a wave maps its block with scalar multiplies.  The functions above stay the definition; tests/block_map_fuzz.cpp holds these
// to them.
//
// UDiv: n / d == mulhi(2 n, mul) >> shift for EVERY n < 2^31, with s = ceil(log2 d), shift = s, mul = ceil(2^(31 + s) / d).
// Proof: mul * d = 2^(31 + s) + e with 0 <= e < d <= 2^s, so n * mul / 2^(31 + s) = n / d + n * e / (d * 2^(31 + s)); the last term
// is below 1 / d because n * e < 2^31 * 2^s, and the fractional part of n / d is at most (d - 1) / d: the floor does not move.
// mul fits 32 bits: 2^(31 + s) / d < 2^32 (d > 2^(s - 1)), and is exactly 2^31 for a power of two, where the whole thing is a shift.
// One form for every divisor, so the kernels carry no branch on the divisor's kind.  d in [1, 2^31]; a larger d divides every n < 2^31 to 0: mul = 0.
struct UDiv { uint32_t mul, shift; };
constexpr uint64_t kUDivBound = 1ull << 31;  // numerators stay below it
inline bool udiv_make(uint32_t d, UDiv &u) {
    u.mul = 0; u.shift = 0;
    if (d == 0) return false;
    if (d > (1u << 31)) return true;  // every n < 2^31 gives 0, and so does mul = 0 (a root_skip the deal never reaches)
    uint32_t s = 0;
    while ((1ull << s) < d) s++;
    u.shift = s;
    u.mul = (uint32_t)(((1ull << (31u + s)) + d - 1u) / d);
    return true;
}
VK_HD uint32_t umulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
VK_HD uint32_t udiv(uint32_t n, UDiv u) { return umulhi32(n << 1, u.mul) >> u.shift; }

// The reciprocals of one launch.  skip / skip_m1 are those of the deal's k and k - 1 (1 when the deal is the plain round robin).
struct BlockMapDesc {
    UDiv per_tile, n_frames, tiles_x, sps, skip, skip_m1;
};
// Filled where the host fills the launch (vk_render.hip, vk_batch.hip).  n_blocks: the launch's logical blocks -- every block index
// the map sees is below it (the grid's padding returns first).  False when a divisor is 0 or a numerator could reach 2^31: the block
// index itself, a tile id (tiles_x * tiles_y stands for "no tile"), or the deal's round slot + slot / (k - 1).
inline bool block_map_make(uint32_t ts, uint32_t tiles_x, uint32_t tiles_y, uint32_t n_frames, uint32_t nranks, uint32_t root_skip, uint64_t n_blocks, BlockMapDesc &m) {
    const uint32_t sps = ts >> 3;
    const uint64_t per_tile = (uint64_t)sps * sps;
    const uint32_t k = (nranks > 1 && root_skip >= 2u) ? root_skip : 0u;
    bool ok = sps != 0 && (ts & 7u) == 0 && per_tile <= kUDivBound && nranks != 0;
    ok = udiv_make((uint32_t)per_tile, m.per_tile) && ok;
    ok = udiv_make(n_frames, m.n_frames) && ok;
    ok = udiv_make(tiles_x, m.tiles_x) && ok;
    ok = udiv_make(sps, m.sps) && ok;
    ok = udiv_make(k ? k : 1u, m.skip) && ok;
    ok = udiv_make(k ? k - 1u : 1u, m.skip_m1) && ok;
    if (!ok) return false;
    if (n_blocks > kUDivBound || (uint64_t)tiles_x * tiles_y >= kUDivBound) return false;
    const uint64_t slot_max = n_blocks / per_tile / n_frames;  // the launch's slots: every slot is below it
    if (k && slot_max + slot_max / (k - 1u) >= kUDivBound) return false;
    return true;
}

// batch_block_split, deal_pos and tile_pixel with the launch's reciprocals: the same results (a single frame is a batch of one)
VK_HD BlockSplit batch_block_split(uint32_t lb, uint32_t per_tile, uint32_t n_frames, bool frame_runs, const BlockMapDesc &m) {
    BlockSplit s;
    const uint32_t g = udiv(lb, m.per_tile);
    s.sub = lb - g * per_tile;
    s.slot = udiv(g, m.n_frames);
    uint32_t fr = g - s.slot * n_frames;
    if (frame_runs) {
        const uint32_t x = fr & 7u, j = fr >> 3, q = n_frames >> 3, rem = n_frames & 7u;
        fr = x * q + (x < rem ? x : rem) + j;
    }
    s.frame = fr;
    return s;
}
VK_HD uint32_t deal_pos(uint32_t rank, uint32_t slot, uint32_t N, uint32_t k, const BlockMapDesc &m) {
    if (k < 2u) return rank + slot * N;
    const uint32_t round = rank ? slot : slot + udiv(slot, m.skip_m1);
    const uint32_t rk = udiv(round, m.skip);
    return round * N - rk + rank - ((round - rk * k) == k - 1u ? 1u : 0u);
}
// (lane 0 gives the 8x8 block's corner)
VK_HD TilePixel tile_pixel(uint32_t ts, uint32_t tiles_x, uint32_t tile, uint32_t sub, uint32_t lane, const BlockMapDesc &m) {
    TilePixel p;
    const uint32_t sps = ts >> 3;
    const uint32_t tty = udiv(tile, m.tiles_x), ttx = tile - tty * tiles_x;
    const uint32_t sy = udiv(sub, m.sps), sx = sub - sy * sps;
    p.lx = sx * 8u + (lane & 7u); p.ly = sy * 8u + (lane >> 3);
    p.rx = ttx * ts + p.lx; p.ry = tty * ts + p.ly;
    return p;
}
// The output index of a block's lane is the index of the block's corner -- wave-uniform, 64 bits -- plus the lane's 32-bit part
// (l >> 3) * pitch + (l & 7), pitch = ts (compact records: compact_pixel_index of the corner) or W (whole frames).  A region origin off the
// screen makes a corner (x0, y0) negative; the pixels such a block stores are on the screen, and for them base + part is frame_pixel_index.
VK_HD int64_t frame_block_base(uint32_t frame, uint32_t W, uint32_t H, int32_t x0, int32_t y0) { return ((int64_t)frame * H + y0) * (int64_t)W + x0; }
VK_HD uint32_t block_lane_part(uint32_t lane, uint32_t pitch) { return (lane >> 3) * pitch + (lane & 7u); }

// compact output of a partition: the (slot, frame) record and the pixel inside it; whole frames: [frame][H][W]
VK_HD uint32_t compact_record(uint32_t slot, uint32_t n_frames, uint32_t frame) { return slot * n_frames + frame; }
VK_HD size_t compact_pixel_index(uint32_t rec, uint32_t ts, uint32_t lx, uint32_t ly) { return (size_t)rec * ((size_t)ts * ts) + (size_t)ly * ts + lx; }
VK_HD size_t frame_pixel_index(uint32_t frame, uint32_t W, uint32_t H, uint32_t x, uint32_t y) { return ((size_t)frame * H + y) * W + x; }
// root side: where pixel (lx, ly) of the tile a rank marched in `slot` of `frame` sits in the gathered [nranks][n_slots][n_frames][ts][ts]
VK_HD size_t gathered_pixel_index(uint32_t rank, uint32_t n_slots, uint32_t slot, uint32_t n_frames, uint32_t frame, uint32_t ts, uint32_t lx, uint32_t ly) {
    return ((((size_t)rank * n_slots + slot) * n_frames + frame) * ts + ly) * ts + lx;
}
// ... and the (slot, frame) record's number in it (VK_WIRE_RGB records are addressed by record, not by pixel)
VK_HD size_t gathered_record(uint32_t rank, uint32_t n_slots, uint32_t slot, uint32_t n_frames, uint32_t frame) { return ((size_t)rank * n_slots + slot) * n_frames + frame; }
// the un-tile kernel's work item: block b of 256 threads moves 512 pixels of one tile of one frame, two adjacent pixels per thread
struct UntileItem { uint32_t frame, tile, l; bool in_range; };
VK_HD UntileItem untile_item(uint32_t b, uint32_t thread, uint32_t ts, uint32_t n_tiles, uint32_t n_frames) {
    UntileItem u;
    const uint32_t chunks = (ts * ts + 511u) / 512u;  // 512-pixel chunks per tile
    const uint32_t chunk = b % chunks; b /= chunks;
    u.tile = b % n_tiles;
    u.frame = b / n_tiles;
    u.l = chunk * 512u + thread * 2u;  // first of this thread's two pixels inside the tile (ts is even)
    u.in_range = u.frame < n_frames && u.l < ts * ts;
    return u;
}
VK_HD uint64_t untile_blocks(uint32_t ts, uint32_t n_tiles, uint32_t n_frames) { return (uint64_t)n_frames * n_tiles * ((ts * ts + 511u) / 512u); }

// what a batch's table block holds, in bytes: FrameDesc[n_frames] | order[n_frames][n_tiles] | pos[n_frames][n_tiles]
VK_HD size_t batch_table_bytes(uint32_t n_frames, size_t n_tiles, size_t frame_desc_bytes) { return (size_t)n_frames * (frame_desc_bytes + 2u * n_tiles * sizeof(uint32_t)); }
VK_HD size_t batch_order_offset(uint32_t n_frames, size_t frame_desc_bytes) { return (size_t)n_frames * frame_desc_bytes; }  // bytes; pos follows at + n_frames * n_tiles words

// ---- the cell layouts (PACKED, PACKED_PAIRS): addressing constants, index tables, and the rule that lets a march read them unclamped --------
// The cell with low-corner voxel i (i in [-1, n - 1] per axis) lives in physical brick (i >> 2) + 1 at in-brick position i & 3; a brick
// holds 64 cells.  CellAddr carries the constants of the byte offset's closed form
//   c0 + bx*kx + by*ky + bz*kz + (ix << sh_x) + (iy << sh_y) + (iz << sh_z),  b = i >> 2
// as the upload computes them (VolumeDesc holds the same fields).  tests/fastpath_fuzz.cpp holds cell_offset_clamped to the plain 64-bit
// form for every shape the upload accepts, under UBSan.
struct CellAddr {
    int64_t kz, c0, max_off;
    int32_t kx, ky;
    uint32_t sh_x, sh_y, sh_z;
};
inline uint32_t cell_bricks(uint32_t n_vox) { return ((n_vox - 1u) >> 2) + 2u; }
inline CellAddr cell_addr_make(uint32_t nbx, uint32_t nby, uint32_t nbz, uint32_t cell_bytes) {
    CellAddr A;
    const int64_t cb = (int64_t)cell_bytes, bxn = nbx, bxyn = (int64_t)nbx * nby;
    const uint64_t n_cells = (uint64_t)nbx * nby * nbz * 64u;
    A.sh_x = cell_bytes == 8 ? 3 : 4;
    A.sh_y = A.sh_x + 2;
    A.sh_z = A.sh_x + 4;
    A.kx = (int32_t)(60 * cb);
    A.ky = (int32_t)((64 * bxn - 16) * cb);
    A.kz = (64 * bxyn - 64) * cb;
    A.c0 = (64 * bxyn + 64 * bxn + 64) * cb;
    A.max_off = (int64_t)(n_cells - 1) * cb;
    return A;
}
// The clamped march's offset (vk_march_parts.hpp: safe_cell_offset): the closed form in 64 bits, clamped into the cell array whatever
// the indices are.  by * ky passes 2^31 on flat volumes of 4 GiB and more (5800 x 5800 x 4 u16: 1450 * 1485568), so that product is
// formed in 64 bits; bx * kx (<= 2049 * 960) and the shifts (<= 8191 << 8) stay far inside 32.
VK_HD int64_t cell_offset_clamped(int64_t kz, int64_t c0, int64_t max_off, int32_t kx, int32_t ky, uint32_t sh_x, uint32_t sh_y, uint32_t sh_z, int ix, int iy, int iz) {
    const int bx = ix >> 2, by = iy >> 2, bz = iz >> 2;
    int64_t off = (int64_t)bz * kz + ((int64_t)by * (int64_t)ky + (int64_t)(bx * kx)) +
                  (int64_t)(int32_t)(((uint32_t)iz << sh_z) + ((uint32_t)iy << sh_y) + ((uint32_t)ix << sh_x)) + c0;  // (shifts of i = -1: on unsigned words)
    return off < 0 ? 0 : (off > max_off ? max_off : off);
}

// Per-axis cell-index tables of the unclamped march (LDS):
//   Tx[i] = 64*((i>>2)+1) + (i&3),  Ty[i] = 64*nbx*((i>>2)+1) + 4*(i&3),  Tz[i] = 64*nbx*nby*((i>>2)+1) + 16*(i&3)
// Each table has n + 3 entries, entry e = i + 2 for i in [-2, n]; the two outer entries repeat their neighbours (clamp), so a position
// up to 1.5 cells outside the box still reads a real cell's entry.  The three tables are stored back to back, padded to whole uint4.
// NOTHING clamps the index itself: cell_march_fast below is what keeps it in [-2, n].
VK_HD uint32_t cell_lut_entries(uint32_t nx, uint32_t ny, uint32_t nz) { return (nx + ny + nz + 9u + 3u) & ~3u; }  // padded to whole uint4
VK_HD uint32_t cell_lut_bytes(uint32_t nx, uint32_t ny, uint32_t nz) { return cell_lut_entries(nx, ny, nz) * 4u; }
// entry e of the back-to-back tables, in cell units (0 in the padding)
VK_HD uint32_t cell_lut_entry(uint32_t e, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t nbx, uint32_t nby) {
    const uint32_t n0 = nx + 3u, n1 = ny + 3u, n2 = nz + 3u;
    if (e >= n0 + n1 + n2) return 0u;
    uint32_t j = e, n = n0, brick_mul = 64u, cell_mul = 1u;
    if (e >= n0 + n1) { j = e - n0 - n1; n = n2; brick_mul = 64u * nbx * nby; cell_mul = 16u; }
    else if (e >= n0) { j = e - n0; n = n1; brick_mul = 64u * nbx; cell_mul = 4u; }
    const uint32_t lo = j > 1u ? j : 1u;
    const uint32_t c = (lo < n - 2u ? lo : n - 2u) - 1u;  // cell coordinate i + 1 in [0, n_vox]
    return brick_mul * ((c + 3u) >> 2) + cell_mul * ((c + 3u) & 3u);
}

constexpr uint32_t kRenderSafeFlag = 4u;       // == VK_RENDER_SAFE (include/vokselis_hip.h; vk_render.hip asserts it)
constexpr uint32_t kCellLutBudget = 16384u;    // bytes of LDS the three tables may take
// May a NAIVE_TRILINEAR march on a cell layout take the unclamped build (SAFE = false: index tables, 32-bit offsets, a plain load of
// the distance byte at the tables' sum)?  One pure function of what the host knows at launch: the array's last offset, the dims, the eye
// (the farthest of a batch), dt_scale and the caller's VK_RENDER_* flags.  It must guarantee that EVERY index a ray looks up -- on every
// trip its f32 loop makes, and (dt_scale <= 1.25) the probe-ahead position one step ahead of each -- lies in [-2, n] on its axis: the
// skip kernels read the distance byte with a plain global load at the tables' sum.  (The request one step ahead in the loops without a
// skip map goes through a bounds-checked load at any dt_scale and is not covered: vk_march.hpp.)
//
// In exact arithmetic a sampled position lies in the box: u = p*n - 0.5 in [-0.5, n - 0.5], floor(u) in [-1, n - 1].  The tables reach
// 1.5 cells further on either side.  The probe-ahead trip looks one step ahead, at most dt_scale <= 1.25 cells (the host drops
// LF_PROBE_AHEAD above that): 0.25 cells are left for everything f32 does to the position, on the worst axis (n <= nmax):
//   set-up    p0 = eye + t0*d, t0 and t1 from the slab test: a few ulp(reach) each, reach = |eye| + 4 >= every t and |eye_i|; 64 ulp(reach).
//   p drift   p += s rounds by <= ulp(2)/2 per trip while |p| < 4; s = fl(d*dt) itself is off by 2^-24 relative, which over a
//             whole ray (<= nmax cells) is nmax * 2^-24 cells and is covered by the factor of two in ulp(2) against ulp(1).
//   t drift   t += dt rounds by <= ulp(reach)/2 per trip, and inside a binade always the same way: after k trips the loop variable is
//             off by up to k*ulp(reach)/2, the loop ends that much late (or early), and the ray has moved on by <= that much on any
//             axis (|d_i| <= 1).
// So k trips move a looked-up position at most 64 ulp(reach) + k*(ulp(reach)/2 + ulp(2)/2) outside the box.  k: the loop makes trip
// k only while t_k < t1, t_k >= t0 + k*(dt - ulp(reach)/2); dt >= dt_scale/nmax, required below to be >= 8 ulp(reach), so
// k < (16/15)*(t1 - t0)/dt, and (t1 - t0)/dt <= nmax/dt_scale because a ray crosses at most n_i cells on the axis that sets dt.
// max_trips = 1.125*nmax/dt_scale + 4 takes the slack.  In double: none of this rounds at a size that matters.
// tests/fastpath_fuzz.cpp replays the f32 loop (primary rays with the probe-ahead position, shadow rays) and holds this rule to it.
inline double cell_march_drift_cells(uint32_t nx, uint32_t ny, uint32_t nz, const float eye[3], float dt_scale) {
    const float reach = std::sqrt(eye[0] * eye[0] + eye[1] * eye[1] + eye[2] * eye[2]) + 4.0f;
    const double nmax = (double)std::max(nx, std::max(ny, nz));
    const double ulp_reach = (double)(std::nextafter(reach, 2.0f * reach) - reach), ulp_2 = (double)(std::nextafter(2.0f, 4.0f) - 2.0f);
    const double max_trips = 1.125 * nmax / (double)dt_scale + 4.0;
    return nmax * (64.0 * ulp_reach + max_trips * (0.5 * ulp_reach + 0.5 * ulp_2));
}
inline bool cell_march_fast(int64_t max_off, uint32_t nx, uint32_t ny, uint32_t nz, const float eye[3], float dt_scale, uint32_t render_flags) {
    if (render_flags & kRenderSafeFlag) return false;
    if (!(max_off + 16 < (1ll << 32))) return false;                    // 32-bit byte offsets
    if (!(cell_lut_bytes(nx, ny, nz) <= kCellLutBudget)) return false;  // the tables' LDS budget
    if (!(dt_scale > 0.0f) || !std::isfinite(dt_scale)) return false;
    const float reach = std::sqrt(eye[0] * eye[0] + eye[1] * eye[1] + eye[2] * eye[2]) + 4.0f;
    if (!std::isfinite(reach)) return false;
    const double nmax = (double)std::max(nx, std::max(ny, nz));
    const double ulp_reach = (double)(std::nextafter(reach, 2.0f * reach) - reach);
    if (!((double)dt_scale / nmax >= 8.0 * ulp_reach)) return false;    // (check_render's guard: the bound on the trips leans on it)
    return cell_march_drift_cells(nx, ny, nz, eye, dt_scale) < 0.25;
}

// ---- host-side geometry of a frame (plain host functions) ---------------------------------------------------------------
constexpr int kModeNaive = 0;  // == VK_MODE_NAIVE_TRILINEAR (include/vokselis_hip.h); the other modes march the [-1, 1]^3 box from the near plane

// The box the NAIVE rays march, in unit-cube coordinates: the unit cube, or the context's clip box (vk_set_clip_box).  The bounds are the
// kernels' f32 values, held in double.
struct ClipBox { double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {1.0, 1.0, 1.0}; };

// Screen-space bounding rectangle of the box (NAIVE mode; the unit cube by default): the 8 corners projected with
// proj_view in double; any corner at or behind the eye plane disables the cull.  Padded by 2 px.
// Pixels outside [x0,x1) x [y0,y1) cannot hit the box.
inline void cull_rect_wh(uint32_t W, uint32_t H, const float *cam, int mode, int32_t r[4], const ClipBox &box = ClipBox()) {
    r[0] = 0; r[1] = 0; r[2] = (int32_t)W; r[3] = (int32_t)H;
    if (mode != kModeNaive) return;
    const float *pv = cam + 4;
    double x0 = 1e300, y0 = 1e300, x1 = -1e300, y1 = -1e300;
    for (int c = 0; c < 8; c++) {
        const double X = (c & 1) ? box.hi[0] : box.lo[0], Y = (c & 2) ? box.hi[1] : box.lo[1], Z = (c & 4) ? box.hi[2] : box.lo[2];
        const double cx = pv[0] * X + pv[4] * Y + pv[8] * Z + pv[12], cy = pv[1] * X + pv[5] * Y + pv[9] * Z + pv[13];
        const double cw = pv[3] * X + pv[7] * Y + pv[11] * Z + pv[15];
        if (!(cw > 1e-6)) return;
        const double sx = (cx / cw * 0.5 + 0.5) * W, sy = (0.5 - cy / cw * 0.5) * H;
        x0 = std::min(x0, sx); x1 = std::max(x1, sx); y0 = std::min(y0, sy); y1 = std::max(y1, sy);
    }
    if (!(std::isfinite(x0) && std::isfinite(x1) && std::isfinite(y0) && std::isfinite(y1))) return;
    // (clamped in double BEFORE the conversion: a corner projected far off screen is a huge double, and int32 of that is undefined)
    r[0] = (int32_t)std::min((double)W, std::max(0.0, std::floor(x0) - 2.0));
    r[1] = (int32_t)std::min((double)H, std::max(0.0, std::floor(y0) - 2.0));
    r[2] = (int32_t)std::max(0.0, std::min((double)W, std::ceil(x1) + 2.0));
    r[3] = (int32_t)std::max(0.0, std::min((double)H, std::ceil(y1) + 2.0));
}

// The box's silhouette on the screen (the unit cube's by default): the convex hull of its 8 projected corners (counter-clockwise in screen
// coordinates, y down), in double.  A pixel's ray hits the box only if the pixel centre lies inside it, so a tile that a
// hull edge separates from it by more than 2 px holds only clear-colour pixels.  The bounding rectangle alone keeps
// 288 of C2's 510 tiles; the hull keeps the ones a ray can actually hit.  n = 0: no hull (a corner behind the eye
// plane, or another mode) -- the rectangle decides alone.
struct CullHull { int n = 0; double x[16], y[16]; };
inline void cull_hull_wh(uint32_t W, uint32_t H, const float *cam, int mode, CullHull &h, const ClipBox &box = ClipBox()) {
    h.n = 0;
    if (mode != kModeNaive) return;
    const float *pv = cam + 4;
    std::pair<double, double> p[8];
    for (int c = 0; c < 8; c++) {
        const double X = (c & 1) ? box.hi[0] : box.lo[0], Y = (c & 2) ? box.hi[1] : box.lo[1], Z = (c & 4) ? box.hi[2] : box.lo[2];
        const double cx = pv[0] * X + pv[4] * Y + pv[8] * Z + pv[12], cy = pv[1] * X + pv[5] * Y + pv[9] * Z + pv[13];
        const double cw = pv[3] * X + pv[7] * Y + pv[11] * Z + pv[15];
        if (!(cw > 1e-6)) return;
        p[c] = {(cx / cw * 0.5 + 0.5) * W, (0.5 - cy / cw * 0.5) * H};
        if (!(std::isfinite(p[c].first) && std::isfinite(p[c].second))) return;
    }
    std::sort(p, p + 8);
    auto cross = [](const std::pair<double, double> &o, const std::pair<double, double> &a, const std::pair<double, double> &b) {
        return (a.first - o.first) * (b.second - o.second) - (a.second - o.second) * (b.first - o.first);
    };
    std::pair<double, double> hull[16];
    int k = 0;
    for (int i = 0; i < 8; i++) { while (k >= 2 && cross(hull[k - 2], hull[k - 1], p[i]) <= 0) k--; hull[k++] = p[i]; }
    for (int i = 6, t = k + 1; i >= 0; i--) { while (k >= t && cross(hull[k - 2], hull[k - 1], p[i]) <= 0) k--; hull[k++] = p[i]; }
    k--;  // (the last point repeats the first)
    if (k < 3) return;  // degenerate (edge-on): the rectangle decides
    h.n = k;
    for (int i = 0; i < k; i++) { h.x[i] = hull[i].first; h.y[i] = hull[i].second; }
}

// true when some hull edge has the whole rectangle [x0,x1] x [y0,y1] more than `pad` pixels on its outer side
inline bool hull_separates(const CullHull &h, double x0, double y0, double x1, double y1, double pad) {
    for (int i = 0; i < h.n; i++) {
        const int j = i + 1 == h.n ? 0 : i + 1;
        const double ex = h.x[j] - h.x[i], ey = h.y[j] - h.y[i];
        const double len = std::sqrt(ex * ex + ey * ey);
        if (!(len > 0)) continue;
        // monotone chain with this cross-product sign walks the hull with its interior on the left: d < 0 is outside
        const double nx = -ey, ny = ex;  // left normal
        const double d0 = nx * (x0 - h.x[i]) + ny * (y0 - h.y[i]), d1 = nx * (x1 - h.x[i]) + ny * (y0 - h.y[i]);
        const double d2 = nx * (x0 - h.x[i]) + ny * (y1 - h.y[i]), d3 = nx * (x1 - h.x[i]) + ny * (y1 - h.y[i]);
        if (std::max(std::max(d0, d1), std::max(d2, d3)) < -pad * len) return true;
    }
    return false;
}

// the tile-level decision, shared by the tile order and vk_tiles_active
inline bool tile_is_inactive(const int32_t cr[4], const CullHull &hull, int64_t x0, int64_t y0, uint32_t ts) {
    return x0 + ts <= cr[0] || x0 >= cr[2] || y0 + ts <= cr[1] || y0 >= cr[3] ||
           (hull.n && hull_separates(hull, (double)x0, (double)y0, (double)(x0 + ts), (double)(y0 + ts), 2.0));
}

// ... under a box: rectangle and hull of the box, and -- when the box is not the unit cube -- of the cube too.  A ray that hits the box hits
// the cube, so either pair may rule a tile out.  The hull test looks along the hull's own edges only; with both pairs a tile the cube's
// silhouette rules out stays ruled out under every box: a clip box never activates a tile.
struct TileCull {
    int32_t cr[4], cube_cr[4];
    CullHull hull, cube_hull;
    bool boxed = false;
};
inline void tile_cull_wh(uint32_t W, uint32_t H, const float *cam, int mode, const ClipBox &box, TileCull &c) {
    cull_rect_wh(W, H, cam, mode, c.cr, box);
    cull_hull_wh(W, H, cam, mode, c.hull, box);
    c.boxed = false;
    for (int k = 0; k < 3; k++) c.boxed = c.boxed || box.lo[k] != 0.0 || box.hi[k] != 1.0;
    if (c.boxed) {
        cull_rect_wh(W, H, cam, mode, c.cube_cr);
        cull_hull_wh(W, H, cam, mode, c.cube_hull);
    }
}
inline bool tile_is_inactive(const TileCull &c, int64_t x0, int64_t y0, uint32_t ts) {
    return tile_is_inactive(c.cr, c.hull, x0, y0, ts) || (c.boxed && tile_is_inactive(c.cube_cr, c.cube_hull, x0, y0, ts));
}

// Tiles are dealt to the launch (and, at N > 1, to the ranks) heaviest first.  The frame is ~70 %
// empty and a dense ray ends after 2 steps while a grazing one takes 513, so with ~10 working waves
// per SIMD the kernel's tail is set by whichever heavy tiles start last; starting them first (and
// round-robining them over ranks) shortens it.  The cost estimate is the nominal step count of a
// G x G grid of rays per tile, from the same camera maths as the kernel, in double precision on the
// host.  It is only a launch order: every tile is rendered by the same kernel whatever its rank.
// (W, H): the frame; (ox, oy, rw, rh): the region the launch covers; dims: the volume's; box: what the NAIVE rays march (a clip box
// shortens the estimate's rays and tightens rectangle and hull).
inline void tile_order(uint32_t W_, uint32_t H_, const uint32_t dims_[3], const float *cam, int mode, int32_t ox, int32_t oy, uint32_t rw, uint32_t rh, uint32_t ts,
                       uint32_t *order, uint32_t *order_pos, uint32_t &order_active, int G, const ClipBox &box = ClipBox()) {
    const uint32_t tx = (rw + ts - 1) / ts, ty = (rh + ts - 1) / ts;
    const size_t n = (size_t)tx * ty;
    const double W = W_, H = H_;
    // tiles that do not touch the cube's screen rectangle hold only clear-colour pixels: they sort last (in index
    // order) and are "inactive" -- never marched, never gathered (the root clears them in vk_untile); no rays for them
    TileCull cull;
    tile_cull_wh(W_, H_, cam, mode, box, cull);
    struct Key { double cost; uint32_t tile; };
    std::vector<Key> act;
    act.reserve(n);
    const float *m = cam + 20;
    const double dims[3] = {(double)std::max(dims_[0], 1u), (double)std::max(dims_[1], 1u), (double)std::max(dims_[2], 1u)};
    uint32_t n_inactive = 0;
    for (uint32_t j = 0; j < ty; j++)
        for (uint32_t i = 0; i < tx; i++) {
            const int64_t x0 = (int64_t)ox + (int64_t)i * ts, y0 = (int64_t)oy + (int64_t)j * ts;
            const uint32_t tile = j * tx + i;
            if (tile_is_inactive(cull, x0, y0, ts)) { order[n - 1 - n_inactive++] = tile; continue; }  // (reversed below)
            double c = 0.0;
            for (int sy = 0; sy < G; sy++)
                for (int sx = 0; sx < G; sx++) {
                    const double px = (double)x0 + (2 * sx + 1) * ts / (2.0 * G), py = (double)y0 + (2 * sy + 1) * ts / (2.0 * G);
                    if (px < 0 || py < 0 || px >= W || py >= H) continue;
                    double e[3], d[3], lo[3], hi[3];
                    if (mode == kModeNaive) {
                        const double X = 2.0 * px / W - 1.0, Y = 1.0 - 2.0 * py / H;
                        const double qw = 1.0 / (m[3] * X + m[7] * Y + m[11] + m[15]);
                        for (int k = 0; k < 3; k++) { e[k] = cam[k]; d[k] = (m[k] * X + m[4 + k] * Y + m[8 + k] + m[12 + k]) * qw - e[k]; }
                        for (int k = 0; k < 3; k++) { lo[k] = box.lo[k]; hi[k] = box.hi[k]; }
                    } else {
                        const double X = 2.0 * px / W - 1.0, Y = (2.0 * py / H - 1.0) * -(H / W);
                        const double aw = 1.0 / (m[3] * X + m[7] * Y + m[15]), bw = 1.0 / (m[3] * X + m[7] * Y + m[11] + m[15]);
                        for (int k = 0; k < 3; k++) {
                            e[k] = (m[k] * X + m[4 + k] * Y + m[12 + k]) * aw;
                            d[k] = (m[k] * X + m[4 + k] * Y + m[8 + k] + m[12 + k]) * bw - e[k];
                        }
                        for (int k = 0; k < 3; k++) { lo[k] = -1.0; hi[k] = 1.0; }
                    }
                    const double len2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
                    if (!(len2 > 0)) continue;
                    // steps = (t1 - t0) / dt with t in units of |d| (the normalisation cancels): dt = min_k 1 / (dims_k |d_k|)
                    double t0 = -1e300, t1 = 1e300, inv_dt = 0.0;
                    for (int k = 0; k < 3; k++) {
                        const double inv = 1.0 / d[k], ta = (lo[k] - e[k]) * inv, tb = (hi[k] - e[k]) * inv;
                        t0 = std::max(t0, std::min(ta, tb));
                        t1 = std::min(t1, std::max(ta, tb));
                        inv_dt = std::max(inv_dt, dims[k] * std::fabs(d[k]));
                    }
                    t0 = std::max(t0, 0.0);
                    if (t1 > t0 && inv_dt > 0) c += (t1 - t0) * inv_dt;
                }
            act.push_back({c, tile});
        }
    const uint32_t n_active = (uint32_t)act.size();
    std::stable_sort(act.begin(), act.end(), [](const Key &a, const Key &b) { return a.cost > b.cost; });
    for (uint32_t q = 0; q < n_active; q++) order[q] = act[q].tile;
    std::reverse(order + n_active, order + n);  // inactive tiles in index order
    // Position q goes to XCD q % 8 (rank q % N first, when the frame is partitioned): dealt straight, bin 0
    // would receive the heaviest tile of every round of 8.  Reverse every other round (snake) so the bins'
    // sums even out; the active tiles stay in front.
    for (size_t g = 8; g + 8 <= n_active; g += 16) std::reverse(order + g, order + g + 8);
    order_active = n_active;
    for (size_t q = 0; q < n; q++) order_pos[order[q]] = (uint32_t)q;
}
}  // namespace vk
