// TEST INFRASTRUCTURE: host build of the mesh pass's shared header (vokselis_amd/csrc/vk_mesh.hpp) under ASan + UBSan, against brute force.
// 1. The table against the geometric orientation rule, derived here without it: for every tetrahedron k and mask 1 .. 14, with the inside
//    vertices at 1 and the outside ones at 0 and the threshold at 0.5, every triangle's edges are crossed edges (one end inside, one
//    outside), the triangles of a mask use every crossed edge, two triangles share exactly one edge and run it in opposite directions, and
//    (p1 - p0) x (p2 - p0) -- second and third vertex swapped for the odd permutations -- has a positive dot product with the direction
//    from the mean inside vertex to the mean outside vertex.  mesh_mask_count is the table's count; mesh_tet_corner is the stated chain.
// 2. mesh_cube_inside / mesh_cube_count against the rule on random corners: a NaN or infinite corner, all inside, all outside give 0.
// 3. f = mesh_edge_f lies in [0, 1] for every crossed edge: all u8 pairs under integer and half-integer thresholds, random u16 and f16
//    pairs (subnormals, -0, the largest halves); mesh_vertex_coord is the stated expression.
// 4. mesh_cube_xyz is a bijection of the chunked cube index onto the box's cubes in x-fastest order, for every chunk size, on its 32-bit
//    and its 64-bit path.
// 5. The chunk, grid and scan arithmetic: mesh_chunk_cubes for every knob, mesh_chunks, mesh_chunk_passes, mesh_totals_padded, mesh_grid, and mesh_scan_host
//    over totals whose sum passes 2^32.
// 6. The validation table: mesh_validate, and the box rules the pass shares with the histogram (vk_box.hpp: voxel_box_ok) with mesh_axis_cubes.
// usage: mesh_fuzz <cases> <seed>; prints "OK (<cases> cases)" or the first violations, and exits non-zero on any.
#include "vk_mesh.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

static uint64_t state;
static uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static long bad = 0;
static void fail(long c, const char *what, double a, double b) { if (bad < 10) printf("case %ld: %s (%a, %a)\n", c, what, a, b); bad++; }

static float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h >> 15) << 31, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 31u) return from_bits(sign | 0x7f800000u | (m << 13));
    if (e != 0u) return from_bits(sign | ((e + 112u) << 23) | (m << 13));
    const float f = (float)m * 0x1p-24f;
    return sign ? -f : f;
}

static const int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

struct Tri { int e[3][2]; };
// the triangles the header emits for (k, mask), vertices in emission order (the swap applied)
static std::vector<Tri> triangles(uint32_t k, uint32_t mask) {
    std::vector<Tri> out;
    const uint32_t row = vk::mesh_table(mask);
    for (uint32_t t = 0; t < vk::mesh_row_count(row); t++) {
        Tri tr;
        for (uint32_t e = 0; e < 3; e++) {
            const uint32_t edge = vk::mesh_row_edge(row, t, e), slot = (vk::mesh_tet_odd(k) && e) ? 3 - e : e;
            tr.e[slot][0] = (int)(edge >> 2);
            tr.e[slot][1] = (int)(edge & 3u);
        }
        out.push_back(tr);
    }
    return out;
}

static void check_table(long c) {
    for (uint32_t k = 0; k < 6; k++) {
        // the stated chain, and the parity from the inversions
        int v[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {1, 1, 1}};
        v[1][PERM[k][0]] = 1; v[2][PERM[k][0]] = 1; v[2][PERM[k][1]] = 1;
        int inv = 0;
        for (int i = 0; i < 3; i++)
            for (int j = i + 1; j < 3; j++) inv += PERM[k][i] > PERM[k][j];
        if (vk::mesh_tet_odd(k) != (inv % 2 == 1)) fail(c, "mesh_tet_odd is not the permutation's parity", k, inv);
        for (uint32_t i = 0; i < 4; i++) {
            if (vk::mesh_tet_corner(k, i) != (uint32_t)(v[i][0] + 2 * v[i][1] + 4 * v[i][2])) fail(c, "mesh_tet_corner is not the chain", k, i);
            if (i < 3 && vk::mesh_perm_axis(k, i) != (uint32_t)PERM[k][i]) fail(c, "mesh_perm_axis", k, i);
        }
        for (uint32_t mask = 0; mask < 16; mask++) {
            const std::vector<Tri> tris = triangles(k, mask);
            if (tris.size() != vk::mesh_mask_count(mask)) fail(c, "mesh_mask_count is not the table's count", k, mask);
            int n_in = 0;
            double in_mean[3] = {0, 0, 0}, out_mean[3] = {0, 0, 0};
            for (int i = 0; i < 4; i++) {
                const bool in = (mask >> i) & 1u;
                n_in += in;
                for (int a = 0; a < 3; a++) (in ? in_mean : out_mean)[a] += v[i][a];
            }
            if (mask == 0u || mask == 15u) { if (!tris.empty()) fail(c, "masks 0 and 15 emit", k, mask); continue; }
            for (int a = 0; a < 3; a++) { in_mean[a] /= n_in; out_mean[a] /= 4 - n_in; }
            const size_t expect = (n_in == 2) ? 2 : 1;
            if (tris.size() != expect) fail(c, "triangle count of a mask", k, mask);
            bool used[4][4] = {};
            for (const Tri &tr : tris) {
                double p[3][3];
                for (int s = 0; s < 3; s++) {
                    const int a = tr.e[s][0], b = tr.e[s][1];
                    if (!(a < b) || (((mask >> a) ^ (mask >> b)) & 1u) == 0u) fail(c, "an edge of the table is not a crossed edge (a, b), a < b", k, mask);
                    used[a][b] = true;
                    for (int x = 0; x < 3; x++) p[s][x] = 0.5 * (v[a][x] + v[b][x]);
                }
                const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]}, w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
                const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
                const double dot = n[0] * (out_mean[0] - in_mean[0]) + n[1] * (out_mean[1] - in_mean[1]) + n[2] * (out_mean[2] - in_mean[2]);
                if (!(dot > 1e-9)) fail(c, "a triangle's normal does not point from inside to outside", 16.0 * k + mask, dot);
            }
            int crossed = 0, covered = 0;
            for (int a = 0; a < 4; a++)
                for (int b = a + 1; b < 4; b++) {
                    const bool x = ((mask >> a) ^ (mask >> b)) & 1u;
                    crossed += x;
                    covered += x && used[a][b];
                    if (used[a][b] && !x) fail(c, "an uncrossed edge is used", k, mask);
                }
            if (crossed != (n_in == 2 ? 4 : 3) || covered != crossed) fail(c, "the triangles do not use every crossed edge", k, mask);
            if (tris.size() == 2) {  // a quad: one shared side, run in opposite directions
                int shared = 0, opposite = 0;
                for (int s = 0; s < 3; s++)
                    for (int t = 0; t < 3; t++) {
                        const int *a0 = tris[0].e[s], *a1 = tris[0].e[(s + 1) % 3], *b0 = tris[1].e[t], *b1 = tris[1].e[(t + 1) % 3];
                        const bool same = a0[0] == b0[0] && a0[1] == b0[1] && a1[0] == b1[0] && a1[1] == b1[1];
                        const bool opp = a0[0] == b1[0] && a0[1] == b1[1] && a1[0] == b0[0] && a1[1] == b0[1];
                        shared += same || opp;
                        opposite += opp;
                    }
                if (shared != 1 || opposite != 1) fail(c, "the two triangles of a mask do not share one side in opposite directions", k, mask);
            }
        }
    }
}

static void check_cube(long c) {
    float v[8];
    const float specials[6] = {NAN, INFINITY, -INFINITY, -0.0f, 0.0f, 1.0f};
    const float iso = (float)(rnd() % 5) * 0.25f;
    for (int i = 0; i < 8; i++) v[i] = (rnd() % 16 == 0) ? specials[rnd() % 6] : (float)(rnd() % 9) * 0.125f;
    bool finite = true;
    uint32_t in = 0;
    for (int i = 0; i < 8; i++) { finite = finite && isfinite(v[i]); in |= (uint32_t)(v[i] >= iso) << i; }
    const uint32_t want = (!finite || in == 0u || in == 255u) ? 0u : in;
    if (vk::mesh_cube_inside(v, iso) != want) fail(c, "mesh_cube_inside", in, want);
    uint32_t n = 0;
    for (uint32_t k = 0; k < 6 && want; k++) {
        uint32_t mask = 0;
        for (uint32_t i = 0; i < 4; i++) mask |= ((want >> vk::mesh_tet_corner(k, i)) & 1u) << i;
        if (mask != vk::mesh_tet_mask(want, k)) fail(c, "mesh_tet_mask", k, mask);
        n += vk::mesh_row_count(vk::mesh_table(mask));
    }
    if (vk::mesh_cube_count(want) != n || n > vk::kMeshCubeMaxTriangles) fail(c, "mesh_cube_count", n, want);
    if (finite && vk::mesh_cube_inside<false>(v, iso) != want) fail(c, "mesh_cube_inside<false> on finite corners", in, want);
}

static void check_f_one(long c, float iso_k, float a, float b) {
    if (!isfinite(a) || !isfinite(b) || ((a >= iso_k) == (b >= iso_k))) return;
    const float f = vk::mesh_edge_f(iso_k, a, b);
    if (!(f >= 0.0f && f <= 1.0f)) fail(c, "f outside [0, 1]", a, b);
    if (a == iso_k && f != 0.0f) fail(c, "vA == iso_k must give f == 0", a, b);
    if (b == iso_k && f != 1.0f) fail(c, "vB == iso_k must give f == 1", a, b);
}
static void check_f_u8(long c) {
    for (int t = 0; t <= 511; t++)  // integer and half-integer thresholds 0 .. 255.5
        for (int a = 0; a < 256; a++)
            for (int b = 0; b < 256; b++) check_f_one(c, 0.5f * (float)t, (float)a, (float)b);
}
static void check_f_random(long c) {
    for (int i = 0; i < 4096; i++) {
        const float a = (float)(rnd() & 0xffffu), b = (float)(rnd() & 0xffffu);
        check_f_one(c, (rnd() & 1u) ? a : ((float)(rnd() & 0x1ffffu) * 0.5f), a, b);
        check_f_one(c, (rnd() & 1u) ? b : (float)(rnd() & 0xffffu), a, b);
        const float x = half_to_float((uint16_t)rnd()), y = half_to_float((uint16_t)rnd()), z = half_to_float((uint16_t)rnd());
        check_f_one(c, z, x, y);
        check_f_one(c, x, x, y);
        check_f_one(c, y, x, y);
    }
    const uint32_t a = (uint32_t)(rnd() % 70000u);
    const float n = (float)(1u + rnd() % 5000u), f = (float)(rnd() >> 40) / 16777216.0f;
    if (vk::mesh_vertex_coord(a, true, f, n) != (((float)a + 0.5f) + f) / n || vk::mesh_vertex_coord(a, false, f, n) != (((float)a + 0.5f) + 0.0f) / n)
        fail(c, "mesh_vertex_coord is not the stated expression", a, f);
}

static void check_mapping(long c) {
    // a small box, every chunk size class: the chunked index enumerates the cubes in x-fastest order, each once
    const uint32_t cx = 1u + (uint32_t)(rnd() % 40u), cy = 1u + (uint32_t)(rnd() % 9u), cz = 1u + (uint32_t)(rnd() % 7u);
    const uint32_t chunk = vk::mesh_chunk_cubes(64u * (1u + (uint32_t)(rnd() % 64u)));
    const uint64_t n = (uint64_t)cx * cy * cz, chunks = vk::mesh_chunks(n, chunk);
    uint64_t next = 0;
    for (uint64_t ch = 0; ch < chunks; ch++)
        for (uint32_t p = 0; p < vk::mesh_chunk_passes(chunk); p++)
            for (uint32_t t = 0; t < vk::kMeshThreads; t++) {
                const uint32_t in_chunk = p * vk::kMeshThreads + t;
                const uint64_t idx = ch * chunk + in_chunk;
                if (in_chunk >= chunk || idx >= n) continue;
                uint32_t x, y, z;
                vk::mesh_cube_xyz(ch * chunk, in_chunk, cx, cy, x, y, z);
                if (idx != next || x != idx % cx || y != (idx / cx) % cy || z != idx / ((uint64_t)cx * cy) || z >= cz) fail(c, "mesh_cube_xyz on a small box", (double)idx, x);
                next++;
            }
    if (next != n) fail(c, "the chunks do not enumerate every cube once", (double)next, (double)n);
    // large boxes: both paths against the plain 64-bit expressions
    for (int i = 0; i < 64; i++) {
        const uint32_t bx = 1u + (uint32_t)(rnd() % 0x7fff0000u), by = 1u + (uint32_t)(rnd() % 70000u), bz = 1u + (uint32_t)(rnd() % 70000u);
        const uint64_t total = (uint64_t)bx * by;  // (a plane; z below keeps the index inside bx by bz)
        uint64_t base = (rnd() % total) + total * (rnd() % bz);
        if (i & 1) base &= 0xffffffffull;
        const uint32_t lane = (uint32_t)(rnd() % 4096u);
        uint32_t x, y, z;
        vk::mesh_cube_xyz(base, lane, bx, by, x, y, z);
        const uint64_t idx = base + lane;
        if (x != idx % bx || y != (idx / bx) % by || z != idx / total) fail(c, "mesh_cube_xyz on a large box", (double)base, lane);
    }
}

static void check_chunks_and_scan(long c) {
    for (uint32_t knob = 0; knob <= 5000u; knob += (knob < 70u || knob > 4090u) ? 1u : 37u) {
        const uint32_t ch = vk::mesh_chunk_cubes(knob);
        if (ch < 64u || ch > 4096u || (ch & 63u) || (knob >= 64u && knob <= 4096u && (ch > knob || knob - ch > 63u)) || (knob == 0u && ch != vk::kMeshChunkCubes))
            fail(c, "mesh_chunk_cubes", knob, ch);
        const uint32_t passes = vk::mesh_chunk_passes(ch);
        if ((uint64_t)passes * vk::kMeshThreads < ch || (uint64_t)(passes - 1u) * vk::kMeshThreads >= ch) fail(c, "mesh_chunk_passes", ch, passes);
        const uint64_t cubes = rnd() % (1ull << (1 + rnd() % 40));
        const uint64_t n = vk::mesh_chunks(cubes, ch);
        if (n * ch < cubes || (n && (n - 1u) * ch >= cubes)) fail(c, "mesh_chunks", (double)cubes, ch);
        const uint64_t padded = vk::mesh_totals_padded(n);
        if (padded < n || padded >= n + vk::kMeshScanPerThread || padded % vk::kMeshScanPerThread) fail(c, "mesh_totals_padded", (double)n, (double)padded);
    }
    for (int i = 0; i < 32; i++) {
        const uint64_t items = rnd() % (1ull << (rnd() % 34));
        const uint32_t cus = (uint32_t)(rnd() % 300u), cap = (rnd() & 1u) ? 0u : 1u + (uint32_t)(rnd() % 5u);
        const uint32_t g = vk::mesh_grid(items, cus, cap);
        const uint64_t full = (uint64_t)(cus ? cus : 1u) * vk::kMeshBlocksPerCU;
        uint64_t want = std::min<uint64_t>(items, full);
        if (cap) want = std::min<uint64_t>(want, cap);
        if (g != std::max<uint64_t>(want, 1u)) fail(c, "mesh_grid", (double)items, g);
    }
    // totals up to a full chunk of 12-triangle cubes: the sum passes 2^32
    const size_t n = 400000u + (size_t)(rnd() % 20000u);
    std::vector<uint32_t> totals(n);
    for (size_t i = 0; i < n; i++) totals[i] = (rnd() % 3u == 0u) ? 0u : (uint32_t)(rnd() % (vk::kMeshChunkMax * vk::kMeshCubeMaxTriangles + 1u));
    totals[n - 1] = vk::kMeshChunkMax * vk::kMeshCubeMaxTriangles;
    std::vector<vk::MeshActive> act(n);
    uint64_t tri = 0;
    const uint64_t na = vk::mesh_scan_host(totals.data(), n, act.data(), tri);
    uint64_t run = 0, k = 0;
    for (size_t i = 0; i < n; i++) {
        if (totals[i]) {
            if (k >= na || act[k].chunk != i || act[k].offset != run || act[k].total != totals[i]) { fail(c, "mesh_scan_host entry", (double)i, (double)k); break; }
            k++;
        }
        run += totals[i];
    }
    if (k != na || tri != run || run <= 0xffffffffull) fail(c, "mesh_scan_host totals", (double)run, (double)na);
}

static void check_validation(long c) {
    if (!vk::mesh_validate(nullptr)) fail(c, "a NULL request is accepted", 0, 0);
    for (float iso : {0.0f, -0.0f, 0.5f, -3.0e38f, 3.0e38f, 1.0e-45f})
        for (uint32_t f : {0u, (uint32_t)VK_MESH_CLIP_BOX}) {
            const vk_mesh_request r = {iso, f};
            if (vk::mesh_validate(&r)) fail(c, "a plain request is refused", iso, f);
        }
    for (float iso : {NAN, INFINITY, -INFINITY}) {
        const vk_mesh_request r = {iso, 0u};
        if (!vk::mesh_validate(&r)) fail(c, "a non-finite iso is accepted", iso, 0);
    }
    for (uint32_t f : {2u, 3u, 4u, 0x80000000u, 0xffffffffu}) {
        const vk_mesh_request r = {0.5f, f};
        if (!vk::mesh_validate(&r)) fail(c, "an unknown flag is accepted", f, 0);
    }
    const uint32_t nx = 1u + (uint32_t)(rnd() % 40u), ny = 1u + (uint32_t)(rnd() % 40u), nz = 1u + (uint32_t)(rnd() % 40u);
    vk_voxel_box b;
    b.x0 = (uint32_t)(rnd() % (nx + 2u)); b.x1 = (uint32_t)(rnd() % (nx + 2u));
    b.y0 = (uint32_t)(rnd() % (ny + 2u)); b.y1 = (uint32_t)(rnd() % (ny + 2u));
    b.z0 = (uint32_t)(rnd() % (nz + 2u)); b.z1 = (uint32_t)(rnd() % (nz + 2u));
    const bool ok = b.x0 <= b.x1 && b.y0 <= b.y1 && b.z0 <= b.z1 && b.x1 <= nx && b.y1 <= ny && b.z1 <= nz;
    if (vk::voxel_box_ok(b, nx, ny, nz) != ok) fail(c, "voxel_box_ok", b.x0, b.x1);
    if (ok) {
        uint64_t cubes = 0;
        for (uint32_t z = b.z0; z + 1u < b.z1; z++)
            for (uint32_t y = b.y0; y + 1u < b.y1; y++)
                for (uint32_t x = b.x0; x + 1u < b.x1; x++) cubes++;
        if (vk::mesh_box_cubes(b) != cubes) fail(c, "mesh_box_cubes", (double)cubes, (double)vk::mesh_box_cubes(b));
    }
    if (vk::mesh_axis_cubes(5u, 5u) || vk::mesh_axis_cubes(5u, 6u) || vk::mesh_axis_cubes(5u, 7u) != 1u || vk::mesh_axis_cubes(0xfffffffeu, 0xffffffffu)) fail(c, "mesh_axis_cubes", 0, 0);
}

int main(int argc, char **argv) {
    const long cases = argc > 1 ? atol(argv[1]) : 200;
    state = argc > 2 ? strtoull(argv[2], nullptr, 0) : 88172645463325252ull;
    if (!state) state = 1;
    check_table(0);
    check_f_u8(0);
    for (long c = 0; c < cases && bad < 10; c++) {
        for (int i = 0; i < 64; i++) check_cube(c);
        check_f_random(c);
        if (c % 8 == 0) check_mapping(c);
        if (c % 64 == 0) check_chunks_and_scan(c);
        check_validation(c);
    }
    if (bad) { printf("%ld violations\n", bad); return 1; }
    printf("OK (%ld cases)\n", cases);
    return 0;
}
