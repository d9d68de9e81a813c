// vk_mesh.hpp -- the isosurface as a triangle mesh by marching tetrahedra (vk_extract_isosurface): the validation of a
// caller's vk_mesh_request, the six tetrahedra of a cube and their 14-row triangle table, the vertex of a crossed edge, the cube-index to
// (x, y, z) mapping and the chunk, grid and scan arithmetic of the kernels, shared by the kernels and their host (vk_launch_mesh.hip) and
// the host fuzz (tests/mesh_fuzz.cpp, plain g++ under ASan / UBSan).  No HIP in the host part.
//
// The rule (the header's text).  A cube is a low-corner voxel (x, y, z) with x0 <= x < x1 - 1 (likewise y, z) of the voxel box; its corners
// are the stored texels as f32 on the kernel's scale.  A corner is inside iff v >= iso_k.  A cube with a NaN or infinite corner, or with all
// corners inside or all outside, emits nothing.  Otherwise tetrahedron k = 0..5 (the k-th permutation pi_k of the axes in lexicographic
// order) has v0 = (0,0,0), v1 = v0 + e[pi_k(0)], v2 = v1 + e[pi_k(1)], v3 = (1,1,1); mask bit i says v_i is inside; the triangles of T[mask]
// are emitted in order, each three tetrahedron edges (a, b), a < b, second and third swapped for the odd permutations k = 1, 2, 5.  The
// vertex on (a, b): A, B the lattice points (A <= B componentwise), f = (iso_k - vA) / (vB - vA), pos.c = (((float)A.c + 0.5f) + (B.c > A.c ?
// f : 0.0f)) / (float)n.c.  Every operation rounded once, nothing fused.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vokselis_hip.h"
#include "vk_box.hpp"

#if defined(__HIPCC__)
#define VK_MESH_HD __host__ __device__ __forceinline__
#else
#define VK_MESH_HD inline
#endif

namespace vk {

// A caller's request.  Returns nullptr, or what is wrong (VK_ERR_INVALID).
inline const char *mesh_validate(const vk_mesh_request *r) {
    if (!r) return "the request is NULL";
    if (!isfinite(r->iso)) return "iso must be finite";
    if (r->flags & ~(uint32_t)VK_MESH_CLIP_BOX) return "unknown flag (VK_MESH_CLIP_BOX)";
    return nullptr;
}

// ---- the tetrahedra ---------------------------------------------------------------------------------------------------------------
// A cube's corner index is i + 2 j + 4 k for the offset (i, j, k): the tap order of a cell.  The axes of pi_k, packed two bits each.
VK_MESH_HD uint32_t mesh_perm_axis(uint32_t k, uint32_t i) {
    // (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x): axis i of permutation k at bits 2 i of entry k
    const uint32_t P = (0x24u) | (0x18u << 6) | (0x21u << 12) | (0x09u << 18) | (0x12u << 24);  // k = 5 below: its entry would not fit a shift of 30 with 6 bits
    return k == 5u ? ((0x06u >> (2u * i)) & 3u) : ((P >> (6u * k + 2u * i)) & 3u);
}
// the cube corner of vertex i (0..3) of tetrahedron k
VK_MESH_HD uint32_t mesh_tet_corner(uint32_t k, uint32_t i) {
    const uint32_t c1 = 1u << mesh_perm_axis(k, 0u), c2 = c1 | (1u << mesh_perm_axis(k, 1u));
    return i == 0u ? 0u : (i == 1u ? c1 : (i == 2u ? c2 : 7u));
}
VK_MESH_HD bool mesh_tet_odd(uint32_t k) { return k == 1u || k == 2u || k == 5u; }

// T[mask]: the triangle count in bits 24..25, triangle t in bits 12 t .. 12 t + 11, its edge e in 4 bits: a in the upper two, b in the lower.
#define VK_MESH_E(a, b) (((uint32_t)(a) << 2) | (uint32_t)(b))
#define VK_MESH_TRI(e0, e1, e2) ((e0) | ((e1) << 4) | ((e2) << 8))
#define VK_MESH_ROW1(t0) ((1u << 24) | (t0))
#define VK_MESH_ROW2(t0, t1) ((2u << 24) | (t0) | ((t1) << 12))
VK_MESH_HD uint32_t mesh_table(uint32_t mask) {
    const uint32_t E01 = VK_MESH_E(0, 1), E02 = VK_MESH_E(0, 2), E03 = VK_MESH_E(0, 3), E12 = VK_MESH_E(1, 2), E13 = VK_MESH_E(1, 3), E23 = VK_MESH_E(2, 3);
    switch (mask & 15u) {
        case 1: return VK_MESH_ROW1(VK_MESH_TRI(E01, E02, E03));
        case 2: return VK_MESH_ROW1(VK_MESH_TRI(E01, E13, E12));
        case 3: return VK_MESH_ROW2(VK_MESH_TRI(E02, E03, E13), VK_MESH_TRI(E02, E13, E12));
        case 4: return VK_MESH_ROW1(VK_MESH_TRI(E02, E12, E23));
        case 5: return VK_MESH_ROW2(VK_MESH_TRI(E01, E23, E03), VK_MESH_TRI(E01, E12, E23));
        case 6: return VK_MESH_ROW2(VK_MESH_TRI(E01, E13, E23), VK_MESH_TRI(E01, E23, E02));
        case 7: return VK_MESH_ROW1(VK_MESH_TRI(E03, E13, E23));
        case 8: return VK_MESH_ROW1(VK_MESH_TRI(E03, E23, E13));
        case 9: return VK_MESH_ROW2(VK_MESH_TRI(E01, E02, E23), VK_MESH_TRI(E01, E23, E13));
        case 10: return VK_MESH_ROW2(VK_MESH_TRI(E01, E23, E12), VK_MESH_TRI(E01, E03, E23));
        case 11: return VK_MESH_ROW1(VK_MESH_TRI(E02, E23, E12));
        case 12: return VK_MESH_ROW2(VK_MESH_TRI(E02, E12, E13), VK_MESH_TRI(E02, E13, E03));
        case 13: return VK_MESH_ROW1(VK_MESH_TRI(E01, E12, E13));
        case 14: return VK_MESH_ROW1(VK_MESH_TRI(E01, E03, E02));
        default: return 0u;  // 0 and 15: nothing
    }
}
VK_MESH_HD uint32_t mesh_row_count(uint32_t row) { return row >> 24; }
// edge e (0..2) of triangle t (0..1) of a row: a = edge >> 2, b = edge & 3
VK_MESH_HD uint32_t mesh_row_edge(uint32_t row, uint32_t t, uint32_t e) { return (row >> (12u * t + 4u * e)) & 15u; }
// the triangles of a mask without the table: one where one or three vertices are inside, two where two are
VK_MESH_HD uint32_t mesh_mask_count(uint32_t mask) {
    const uint32_t pc = (uint32_t)__builtin_popcount(mask & 15u);
    return pc == 2u ? 2u : (pc & 1u);
}

// `inside`: bit c set iff corner c of the cube is inside.  The mask of tetrahedron k.
VK_MESH_HD uint32_t mesh_tet_mask(uint32_t inside, uint32_t k) {
    return ((inside >> mesh_tet_corner(k, 0u)) & 1u) | (((inside >> mesh_tet_corner(k, 1u)) & 1u) << 1) | (((inside >> mesh_tet_corner(k, 2u)) & 1u) << 2) |
           (((inside >> mesh_tet_corner(k, 3u)) & 1u) << 3);
}
// The inside bits of a cube that emits, 0 of one that does not: a NaN or infinite corner, all inside (v >= iso_k), all outside.
// CAN_BE_NON_FINITE: false for the integer formats, whose texels are finite by construction -- the test is left out.
template <bool CAN_BE_NON_FINITE = true>
VK_MESH_HD uint32_t mesh_cube_inside(const float (&v)[8], float iso_k) {
    float mn = v[0], mx = v[0];
    bool finite = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 8; c++) {
        if (CAN_BE_NON_FINITE) finite = finite && (fabsf(v[c]) < INFINITY);  // false for a NaN too
        mn = fminf(mn, v[c]);
        mx = fmaxf(mx, v[c]);
    }
    if (!finite || mn >= iso_k || !(mx >= iso_k)) return 0u;
    uint32_t in = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < 8; c++) in |= (v[c] >= iso_k ? 1u : 0u) << c;
    return in;
}
// the triangles of a cube from its inside bits
VK_MESH_HD uint32_t mesh_cube_count(uint32_t inside) {
    if (inside == 0u) return 0u;
    uint32_t n = 0u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < 6u; k++) n += mesh_mask_count(mesh_tet_mask(inside, k));
    return n;
}
constexpr uint32_t kMeshCubeMaxTriangles = 12;

// The vertex on the edge from lattice point A (value vA) to B (value vB), A <= B componentwise: the fraction, and one coordinate (a: A's
// index on the axis; moves: B lies one further on it; n: the volume's extent on it).
VK_MESH_HD float mesh_edge_f(float iso_k, float vA, float vB) { return (iso_k - vA) / (vB - vA); }
VK_MESH_HD float mesh_vertex_coord(uint32_t a, bool moves, float f, float n) { return (((float)a + 0.5f) + (moves ? f : 0.0f)) / n; }

// ---- cubes, chunks, grids -----------------------------------------------------------------------------------------------------------
// the cubes of a box per axis: a box thinner than 2 voxels has none
VK_MESH_HD uint32_t mesh_axis_cubes(uint32_t a0, uint32_t a1) { return a1 > a0 + 1u ? a1 - a0 - 1u : 0u; }
inline uint64_t mesh_box_cubes(const vk_voxel_box &b) {
    return (uint64_t)mesh_axis_cubes(b.x0, b.x1) * (uint64_t)mesh_axis_cubes(b.y0, b.y1) * (uint64_t)mesh_axis_cubes(b.z0, b.z1);
}
// Cube `base + lane` of the box-ordered index (x fastest, then y, then z) as offsets (x, y, z) from the box's low corner; cx, cy: cubes
// per axis (>= 1).  In two steps, so that a kernel divides `base` -- a chunk's first cube, uniform over a workgroup and all its passes --
// once per chunk: mesh_cube_base (32-bit divisions wherever base fits), then per lane two 32-bit divisions.  lane < 2^16 and cx < 2^32 -
// 2^16 keep bx + lane and by + q within 32 bits (a volume axis stays below 2^31).
struct MeshCubeBase {
    uint32_t bx, by, bz;
};
VK_MESH_HD MeshCubeBase mesh_cube_base(uint64_t base, uint32_t cx, uint32_t cy) {
    MeshCubeBase B;
    if ((base >> 32) == 0u) {
        const uint32_t b = (uint32_t)base, row = b / cx;
        B.bx = b - row * cx;
        B.bz = row / cy;
        B.by = row - B.bz * cy;
    } else {
        const uint64_t row = base / cx, pl = row / cy;
        B.bx = (uint32_t)(base - row * cx);
        B.by = (uint32_t)(row - pl * cy);
        B.bz = (uint32_t)pl;
    }
    return B;
}
VK_MESH_HD void mesh_cube_xyz(const MeshCubeBase &B, uint32_t lane, uint32_t cx, uint32_t cy, uint32_t &x, uint32_t &y, uint32_t &z) {
    const uint32_t t = B.bx + lane, q = t / cx;
    x = t - q * cx;
    const uint32_t u = B.by + q, q2 = u / cy;
    y = u - q2 * cy;
    z = B.bz + q2;
}
VK_MESH_HD void mesh_cube_xyz(uint64_t base, uint32_t lane, uint32_t cx, uint32_t cy, uint32_t &x, uint32_t &y, uint32_t &z) {
    mesh_cube_xyz(mesh_cube_base(base, cx, cy), lane, cx, cy, x, y, z);
}

constexpr uint32_t kMeshThreads = 256;          // a workgroup: four waves, one cube per lane and pass
constexpr uint32_t kMeshBlocksPerCU = 8;
constexpr uint32_t kMeshChunkCubes = 1024;      // the unit of the scan: a contiguous range of the box-ordered cube index
constexpr uint32_t kMeshChunkMin = 64, kMeshChunkMax = 4096;
constexpr uint32_t kMeshScanThreads = 1024;     // the scan pass: one workgroup ...
constexpr uint32_t kMeshScanPerThread = 8;      // ... a thread takes 8 consecutive chunk totals (two 16-byte loads): a tile of 8192 per pass
// entries of the totals array: the chunks rounded up to a thread's 8, so that its loads stay inside (the entries behind the last chunk are
// never written and are masked after the load)
VK_MESH_HD uint64_t mesh_totals_padded(uint64_t n_chunks) { return (n_chunks + kMeshScanPerThread - 1u) / kMeshScanPerThread * kMeshScanPerThread; }

// the chunk in force: the debug knob (0: the default) rounded down to a multiple of 64 within [64, 4096]
VK_MESH_HD uint32_t mesh_chunk_cubes(uint32_t knob) {
    uint32_t c = knob ? knob : kMeshChunkCubes;
    c = c < kMeshChunkMin ? kMeshChunkMin : (c > kMeshChunkMax ? kMeshChunkMax : c);
    return c & ~63u;
}
VK_MESH_HD uint64_t mesh_chunks(uint64_t cubes, uint32_t chunk) { return (cubes + chunk - 1u) / chunk; }
// passes of kMeshThreads cubes a workgroup makes over a chunk (block-uniform)
VK_MESH_HD uint32_t mesh_chunk_passes(uint32_t chunk) { return (chunk + kMeshThreads - 1u) / kMeshThreads; }
// a chunk's total fits 32 bits: 4096 cubes x 12 triangles
static_assert((uint64_t)kMeshChunkMax * kMeshCubeMaxTriangles < 0xffffffffull, "a chunk's total is a u32");
// blocks of a launch over `items` chunks: a block per chunk, at most what the device holds at once, at most the debug cap (0: none), at least 1
VK_MESH_HD uint32_t mesh_grid(uint64_t items, uint32_t cus, uint32_t max_blocks) {
    uint64_t g = items;
    const uint64_t full = (uint64_t)(cus ? cus : 1u) * kMeshBlocksPerCU;
    g = g > full ? full : g;
    if (max_blocks && g > max_blocks) g = max_blocks;
    return g < 1u ? 1u : (uint32_t)g;
}

// What the scan pass leaves per chunk with a non-zero total, in chunk order, and its header.
struct MeshActive {
    uint64_t offset;  // triangles before the chunk
    uint32_t chunk, total;
};
struct MeshScanHeader {
    uint64_t n_triangles, n_active;
};
// The scan on the host, as the kernel must leave it: returns the number of active chunks written to `act`.
inline uint64_t mesh_scan_host(const uint32_t *totals, uint64_t n_chunks, MeshActive *act, uint64_t &n_triangles) {
    uint64_t run = 0u, na = 0u;
    for (uint64_t c = 0; c < n_chunks; c++) {
        if (totals[c]) { act[na].offset = run; act[na].chunk = (uint32_t)c; act[na].total = totals[c]; na++; }
        run += totals[c];
    }
    n_triangles = run;
    return na;
}
constexpr uint64_t kMeshMaxChunks = 0xffffffffull;  // a chunk index is a u32 (64 Gi cubes at the smallest chunk)

}  // namespace vk
