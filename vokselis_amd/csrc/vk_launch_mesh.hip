// vk_launch_mesh.hip -- the isosurface as a triangle mesh by marching tetrahedra (vk_extract_isosurface).  A kernel
// family of its own: a deterministic count, scan and emit stream compaction over the cubes of a voxel box, no ray and no atomic append.
// The tetrahedra, the table, the vertex formula, the cube mapping and all launch arithmetic are vk_mesh.hpp's, shared with the host fuzz.
//
// Count.  One cube per lane and pass, four passes' loads in flight.  Where a cell is, its load, its taps as f32 and a LINEAR element are
// vk_texel.hpp's.  On the cell layouts the cell of the cube's low-corner voxel holds its eight corners: one load.  LINEAR reads
// the two rows of two planes with plain loads -- neighbouring lanes are neighbouring cubes of a row, so the eight loads of a wave fall into
// the same few cache lines and every texel comes from memory once.  A cube is rejected by the minimum and maximum of its corners before the
// tetrahedra are looked at.  A workgroup takes a chunk -- a contiguous range of the box-ordered cube index -- per trip of its grid-stride
// loop, a lane sums its cubes' triangle counts over the chunk's passes, and one workgroup prefix (a wave prefix by __shfl_up, the four waves
// through LDS) gives the chunk's total.
// Scan.  One workgroup turns the totals into exclusive u64 offsets, a tile of 8192 chunks per pass, and compacts the chunks that have a
// triangle into a list (chunk, offset, total) in chunk order; its header holds n and the list's length.
// Emit.  Launched over that list only.  A workgroup re-classifies the cubes of its chunk, forms the in-chunk exclusive offsets pass by pass
// with the same prefix, and every lane writes its cube's triangles at offset < cap.
//
// Loop bounds are block-uniform wherever a barrier stands.  Plain C++; no inline assembly.
#include "vk_launch.hpp"
#include "vk_mesh.hpp"
#include "vk_texel.hpp"

using namespace vk;

struct MeshDesc {
    float iso_k;
    uint32_t chunk, passes;       // cubes per chunk, passes of kMeshThreads cubes over it
    uint32_t x0, y0, z0;          // the box's low corner
    uint32_t cx, cy, cz;          // cubes per axis
    uint32_t pad;
    float fnx, fny, fnz;          // the volume's dimensions as f32
    uint32_t pad2;
    uint64_t n_cubes, n_chunks;
};
static_assert(sizeof(MeshDesc) % 8 == 0 && pass_kernargs_fit<MeshDesc>, "mesh kernels: VolumeDesc + MeshDesc");

// The eight corners of the cube with low-corner voxel (x, y, z), in two steps so that a kernel can issue several cubes' loads before it looks
// at the first: mesh_fetch loads the raw words, mesh_unpack turns them into f32, corner i + 2 j + 4 k at v[...].  x + 1 < nx (likewise y,
// z): a cube's corners are voxels of the volume, so the cell's taps are stored texels, never the clamp's duplicates, and the LINEAR
// indices lie inside the array.
template <int VOL>
struct MeshTaps {
    uint32_t w[is_cell_layout(VOL) ? cell_words(VOL) : 8];  // a cell's words, or the eight texels' bits
};
template <int VOL>
__device__ __forceinline__ void mesh_fetch(const VolumeDesc &V, uint32_t x, uint32_t y, uint32_t z, MeshTaps<VOL> &T) {
    if constexpr (is_cell_layout(VOL)) load_cell<VOL>(cell_ptr(V, x, y, z), T.w);
    else {
        const uint64_t row = V.nx, plane = (uint64_t)V.nx * V.ny;
        const uint64_t i0 = voxel_index(x, y, z, V.nx, V.ny);
#pragma unroll
        for (int b = 0; b < 8; b++) T.w[b] = linear_texel_bits<VOL>(V.data, i0 + (b & 1) + ((b >> 1) & 1) * row + (b >> 2) * plane);
    }
}
template <int VOL>
__device__ __forceinline__ void mesh_unpack(const MeshTaps<VOL> &T, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int b = VOL == VOL_P8 ? (i >> 1) + 4 * (i & 1) : i;  // (P8: the two words' bytes in turn -- the count kernel's schedule follows the order)
        if constexpr (is_cell_layout(VOL)) v[b] = cell_tap_f32<VOL>(T.w, (uint32_t)b);
        else v[b] = texel_f32<VOL>(T.w[b]);
    }
}
template <int VOL>
__device__ __forceinline__ void mesh_corners(const VolumeDesc &V, uint32_t x, uint32_t y, uint32_t z, float (&v)[8]) {
    MeshTaps<VOL> T;
    mesh_fetch<VOL>(V, x, y, z, T);
    mesh_unpack<VOL>(T, v);
}

// The lane's cube of pass p of the chunk that starts at cube c0 (B: mesh_cube_base of c0, formed once per chunk): whether it exists, its
// low-corner voxel, its inside bits (0: emits nothing).
template <int VOL>
__device__ __forceinline__ uint32_t mesh_classify(const VolumeDesc &V, const MeshDesc &D, uint64_t c0, const MeshCubeBase &B, uint32_t p, uint32_t &x, uint32_t &y, uint32_t &z, float (&v)[8]) {
    const uint32_t in_chunk = p * kMeshThreads + threadIdx.x;
    if (in_chunk >= D.chunk || c0 + in_chunk >= D.n_cubes) return 0u;
    mesh_cube_xyz(B, in_chunk, D.cx, D.cy, x, y, z);
    x += D.x0; y += D.y0; z += D.z0;
    mesh_corners<VOL>(V, x, y, z, v);
    return mesh_cube_inside<is_f16_kind(VOL)>(v, D.iso_k);
}

// The workgroup's exclusive prefix of c in thread order, and the total.  Two barriers: w_tot is free again on return.
__device__ __forceinline__ uint32_t mesh_block_prefix(uint32_t c, uint32_t *w_tot, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = c;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63u) w_tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0u;
    total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kMeshThreads / 64u; w++) {
        const uint32_t t = w_tot[w];
        before += w < wave ? t : 0u;
        total += t;
    }
    __syncthreads();
    return before + inc - c;
}

// The count pass is bound by the latency of its loads, not by their bytes: kMeshCountUnroll passes of a chunk are taken together, the loads
// of all of them issued before the first is looked at.  So that no load stands behind a divergent branch, a lane without a cube (behind the
// chunk's or the box's last one) reads the chunk's last cube instead and drops its count.
constexpr uint32_t kMeshCountUnroll = 4;

template <int VOL>
__global__ __launch_bounds__(kMeshThreads) void mesh_count_kernel(const VolumeDesc V, const MeshDesc D, uint32_t *__restrict__ totals) {
    __shared__ uint32_t w_tot[kMeshThreads / 64u];
    for (uint64_t ch = blockIdx.x; ch < D.n_chunks; ch += gridDim.x) {  // block-uniform
        const uint64_t c0 = ch * D.chunk, left = D.n_cubes - c0;    // (left >= 1: the chunk exists)
        const uint32_t live = left < D.chunk ? (uint32_t)left : D.chunk;  // the chunk's cubes
        const MeshCubeBase B = mesh_cube_base(c0, D.cx, D.cy);
        uint32_t mine = 0u;
        for (uint32_t p = 0; p < D.passes; p += kMeshCountUnroll) {
            MeshTaps<VOL> taps[kMeshCountUnroll];
            bool has[kMeshCountUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kMeshCountUnroll; u++) {
                const uint32_t in_chunk = (p + u) * kMeshThreads + threadIdx.x;
                has[u] = in_chunk < live;
                uint32_t x, y, z;
                mesh_cube_xyz(B, has[u] ? in_chunk : live - 1u, D.cx, D.cy, x, y, z);
                mesh_fetch<VOL>(V, x + D.x0, y + D.y0, z + D.z0, taps[u]);
            }
#pragma unroll
            for (uint32_t u = 0; u < kMeshCountUnroll; u++) {
                float v[8];
                mesh_unpack<VOL>(taps[u], v);
                const uint32_t n = mesh_cube_count(mesh_cube_inside<is_f16_kind(VOL)>(v, D.iso_k));
                mine += has[u] ? n : 0u;
            }
        }
        uint32_t total;
        (void)mesh_block_prefix(mine, w_tot, total);
        if (threadIdx.x == 0u) totals[ch] = total;
    }
}

__device__ __forceinline__ float mesh_sel4(float a0, float a1, float a2, float a3, uint32_t i) { return i == 0u ? a0 : (i == 1u ? a1 : (i == 2u ? a2 : a3)); }
__device__ __forceinline__ uint32_t mesh_sel4u(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t i) { return i == 0u ? a0 : (i == 1u ? a1 : (i == 2u ? a2 : a3)); }

// the triangles of one cube, from triangle index `at` on; triangles at cap and beyond are not written
__device__ __forceinline__ void mesh_emit_cube(const MeshDesc &D, uint32_t inside, uint32_t x, uint32_t y, uint32_t z, const float (&v)[8], uint64_t at, uint64_t cap, float *__restrict__ out) {
#pragma unroll
    for (uint32_t k = 0; k < 6u; k++) {
        const uint32_t c0 = mesh_tet_corner(k, 0u), c1 = mesh_tet_corner(k, 1u), c2 = mesh_tet_corner(k, 2u), c3 = mesh_tet_corner(k, 3u);  // compile-time
        const uint32_t row = mesh_table(mesh_tet_mask(inside, k));
        const uint32_t nt = mesh_row_count(row);
        for (uint32_t t = 0; t < nt; t++, at++) {
            if (at >= cap) return;
            float *tri = out + at * 9u;
#pragma unroll
            for (uint32_t e = 0; e < 3u; e++) {
                const uint32_t edge = mesh_row_edge(row, t, e), a = edge >> 2, b = edge & 3u;
                const float vA = mesh_sel4(v[c0], v[c1], v[c2], v[c3], a), vB = mesh_sel4(v[c0], v[c1], v[c2], v[c3], b);
                const uint32_t ca = mesh_sel4u(c0, c1, c2, c3, a), cb = mesh_sel4u(c0, c1, c2, c3, b);
                const float f = mesh_edge_f(D.iso_k, vA, vB);
                const uint32_t slot = (mesh_tet_odd(k) && e != 0u) ? 3u - e : e;
                const uint32_t mv = cb & ~ca;  // the axes on which B lies one further than A
                tri[3u * slot + 0u] = mesh_vertex_coord(x + (ca & 1u), (mv & 1u) != 0u, f, D.fnx);
                tri[3u * slot + 1u] = mesh_vertex_coord(y + ((ca >> 1) & 1u), (mv & 2u) != 0u, f, D.fny);
                tri[3u * slot + 2u] = mesh_vertex_coord(z + ((ca >> 2) & 1u), (mv & 4u) != 0u, f, D.fnz);
            }
        }
    }
}

template <int VOL>
__global__ __launch_bounds__(kMeshThreads) void mesh_emit_kernel(const VolumeDesc V, const MeshDesc D, const MeshActive *__restrict__ act, const uint64_t n_active,
                                                                 float *__restrict__ out, const uint64_t cap) {
    __shared__ uint32_t w_tot[kMeshThreads / 64u];
    for (uint64_t i = blockIdx.x; i < n_active; i += gridDim.x) {  // block-uniform
        const MeshActive a = act[i];
        if (a.offset >= cap) break;  // the list is in chunk order: every later chunk lies behind the cap too (block-uniform)
        const uint64_t c0 = (uint64_t)a.chunk * D.chunk;
        const MeshCubeBase B = mesh_cube_base(c0, D.cx, D.cy);
        uint64_t run = a.offset;
        for (uint32_t p = 0; p < D.passes; p++) {
            uint32_t x = 0u, y = 0u, z = 0u;
            float v[8];
            const uint32_t inside = mesh_classify<VOL>(V, D, c0, B, p, x, y, z, v);
            uint32_t total;
            const uint32_t before = mesh_block_prefix(mesh_cube_count(inside), w_tot, total);
            if (inside) mesh_emit_cube(D, inside, x, y, z, v, run + before, cap, out);
            run += total;
        }
    }
}

// One workgroup: exclusive u64 offsets of the chunk totals and the list of the chunks that have a triangle, in chunk order.  A pass of the
// loop is a dependent load, two barriers and a store -- a few microseconds -- so a thread takes kMeshScanPerThread consecutive totals per
// pass: 1 M chunks (1024^3) are 128 passes.  totals holds mesh_totals_padded(n_chunks) entries.
__global__ __launch_bounds__(kMeshScanThreads) void mesh_scan_kernel(const uint32_t *__restrict__ totals, const uint64_t n_chunks, MeshActive *__restrict__ act, MeshScanHeader *__restrict__ hdr) {
    constexpr uint32_t W = kMeshScanThreads / 64u, K = kMeshScanPerThread;
    __shared__ unsigned long long w_sum[W];
    __shared__ uint32_t w_act[W];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_padded = mesh_totals_padded(n_chunks);
    uint64_t run = 0u, n_act = 0u;
    for (uint64_t first = 0; first < n_chunks; first += (uint64_t)kMeshScanThreads * K) {  // block-uniform
        const uint64_t i0 = first + (uint64_t)threadIdx.x * K;  // a multiple of K: the thread's K entries lie inside the array or all behind it
        uint32_t t[K];
#pragma unroll
        for (uint32_t j = 0; j < K; j += 4u) {
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (i0 < n_padded) q = *reinterpret_cast<const uint4 *>(totals + i0 + j);
            t[j] = q.x; t[j + 1u] = q.y; t[j + 2u] = q.z; t[j + 3u] = q.w;
        }
        unsigned long long mine = 0u;
        uint32_t mine_act = 0u;
#pragma unroll
        for (uint32_t j = 0; j < K; j++) {
            if (i0 + j >= n_chunks) t[j] = 0u;  // (the padding was never written)
            mine += t[j];
            mine_act += t[j] ? 1u : 0u;
        }
        unsigned long long inc = mine;
        uint32_t inc_act = mine_act;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const unsigned long long u = (unsigned long long)__shfl_up((long long)inc, d);
            const uint32_t a = (uint32_t)__shfl_up((int)inc_act, d);
            if (lane >= d) { inc += u; inc_act += a; }
        }
        if (lane == 63u) { w_sum[wave] = inc; w_act[wave] = inc_act; }
        __syncthreads();
        unsigned long long before = 0u, total = 0u;
        uint32_t abefore = 0u, atotal = 0u;
#pragma unroll
        for (uint32_t w = 0; w < W; w++) {
            const unsigned long long s = w_sum[w];
            const uint32_t n = w_act[w];
            before += w < wave ? s : 0ull;
            abefore += w < wave ? n : 0u;
            total += s;
            atotal += n;
        }
        __syncthreads();
        uint64_t off = run + before + inc - mine, k = n_act + abefore + inc_act - mine_act;
#pragma unroll
        for (uint32_t j = 0; j < K; j++) {
            if (t[j]) {
                MeshActive a;
                a.offset = off;
                a.chunk = (uint32_t)(i0 + j);
                a.total = t[j];
                act[k++] = a;
            }
            off += t[j];
        }
        run += total;
        n_act += atotal;
    }
    if (threadIdx.x == 0u) { hdr->n_triangles = run; hdr->n_active = n_act; }
}

int vk_extract_isosurface(vk_ctx *ctx, const vk_mesh_request *req, const vk_voxel_box *box, float *triangles, uint64_t cap_triangles, uint64_t *n_triangles) {
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = mesh_validate(req)) return fail(ctx, VK_ERR_INVALID, std::string("vk_extract_isosurface: ") + why);
    if (!n_triangles) return fail(ctx, VK_ERR_INVALID, "vk_extract_isosurface: n_triangles is NULL");
    if (int rc = pass_needs(ctx, PASS_NEEDS_VOLUME, "vk_extract_isosurface", "mesh")) return rc;
    vk_voxel_box B;
    if (int rc = pass_voxel_box(ctx, "vk_extract_isosurface", "VK_MESH_CLIP_BOX", box, (req->flags & VK_MESH_CLIP_BOX) != 0u, B)) return rc;
    if (int rc = pass_needs(ctx, PASS_NEEDS_SCALAR_KIND, "vk_extract_isosurface", "mesh")) return rc;

    MeshDesc D{};
    D.iso_k = iso_k(req->iso, format_scale(ctx->format));
    D.chunk = mesh_chunk_cubes(ctx->mesh_chunk_cubes);
    D.passes = mesh_chunk_passes(D.chunk);
    D.x0 = B.x0; D.y0 = B.y0; D.z0 = B.z0;
    D.cx = mesh_axis_cubes(B.x0, B.x1); D.cy = mesh_axis_cubes(B.y0, B.y1); D.cz = mesh_axis_cubes(B.z0, B.z1);
    D.fnx = (float)ctx->nx; D.fny = (float)ctx->ny; D.fnz = (float)ctx->nz;
    D.n_cubes = mesh_box_cubes(B);
    D.n_chunks = mesh_chunks(D.n_cubes, D.chunk);
    if (D.n_cubes == 0u) { *n_triangles = 0u; return VK_OK; }
    if (D.n_chunks > kMeshMaxChunks) return fail(ctx, VK_ERR_INVALID, "vk_extract_isosurface: the box holds more chunks than a 32-bit index");

    const int kind = ctx->vol_kind;
    const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
    const VolumeDesc V = volume_desc(ctx);

    // one work buffer: the header, the list of active chunks, the chunk totals
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t work_bytes = sizeof(MeshScanHeader) + (size_t)D.n_chunks * sizeof(MeshActive) + (size_t)mesh_totals_padded(D.n_chunks) * sizeof(uint32_t);
    DeviceTemp work;
    PassCall call{ctx, "vk_extract_isosurface"};
    if (int rc = call.alloc(work, work_bytes, "the work buffer")) return rc;
    MeshScanHeader *d_hdr = reinterpret_cast<MeshScanHeader *>(work.p);
    MeshActive *d_act = reinterpret_cast<MeshActive *>(d_hdr + 1);
    uint32_t *d_totals = reinterpret_cast<uint32_t *>(d_act + D.n_chunks);
    call.phase(false, [&] {
        with_scalar_kind(kind, [&](auto VOL) {
            hipLaunchKernelGGL(mesh_count_kernel<VOL()>, dim3(mesh_grid(D.n_chunks, cus, ctx->mesh_max_blocks)), dim3(kMeshThreads), 0, ctx->stream, V, D, d_totals);
        });
    });
    call.phase(false, [&] { hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kMeshScanThreads), 0, ctx->stream, (const uint32_t *)d_totals, D.n_chunks, d_act, d_hdr); });
    MeshScanHeader hdr{};
    call.download(&hdr, d_hdr, sizeof(hdr));
    if (int rc = call.finish()) return rc;

    const uint64_t n_write = hdr.n_triangles < cap_triangles ? hdr.n_triangles : cap_triangles;
    if (triangles && n_write) {  // (no triangle to write: no emit launch)
        const size_t out_bytes = (size_t)n_write * 9u * sizeof(float);
        DeviceTemp d_out;
        if (int rc = call.alloc(d_out, out_bytes, "the output buffer")) return rc;
        call.phase(false, [&] {
            with_scalar_kind(kind, [&](auto VOL) {
                hipLaunchKernelGGL(mesh_emit_kernel<VOL()>, dim3(mesh_grid(hdr.n_active, cus, ctx->mesh_max_blocks)), dim3(kMeshThreads), 0, ctx->stream, V, D, (const MeshActive *)d_act,
                                   hdr.n_active, reinterpret_cast<float *>(d_out.p), n_write);
            });
        });
        call.download(triangles, d_out.p, out_bytes);
        if (int rc = call.finish()) return rc;
    }
    *n_triangles = hdr.n_triangles;
    return VK_OK;
}
