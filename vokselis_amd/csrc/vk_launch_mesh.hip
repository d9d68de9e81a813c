// vk_launch_mesh.hip -- the isosurface as a triangle mesh by marching tetrahedra (vk_extract_isosurface).  A kernel
// family of its own: a deterministic count, scan and emit stream compaction over the cubes of a voxel box, no ray and no atomic append.
// The tetrahedra, the table, the vertex formula, the cube mapping and all launch arithmetic are vk_mesh.hpp's, shared with the host fuzz.
//
// Count.  One cube per lane and pass, four passes' loads in flight.  On the cell layouts the cell of the cube's low-corner voxel holds its eight corners: one load.  LINEAR reads
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
static_assert(sizeof(MeshDesc) % 8 == 0 && sizeof(VolumeDesc) + sizeof(MeshDesc) + 256 <= 4096, "mesh kernels: VolumeDesc + MeshDesc");

// the byte offset of the cell with low-corner voxel (ix, iy, iz) (vk_common.hpp: VolumeDesc), held inside the cell array
__device__ __forceinline__ int64_t mesh_cell_offset(const VolumeDesc &V, uint32_t ix, uint32_t iy, uint32_t iz) {
    const int64_t off = (int64_t)(iz >> 2) * V.kz + (int64_t)(iy >> 2) * (int64_t)V.ky + (int64_t)(ix >> 2) * (int64_t)V.kx +
                        (((int64_t)iz << V.sh_z) + ((int64_t)iy << V.sh_y) + ((int64_t)ix << V.sh_x)) + V.c0;
    return off < 0 ? 0 : (off > V.max_off ? V.max_off : off);
}

template <int VOL>
__device__ __forceinline__ float mesh_texel16(uint32_t bits) {
    if constexpr (VOL == VOL_LINEAR_F16 || VOL == VOL_PF16) return h2f(bits & 0xffffu);
    else return (float)(bits & 0xffffu);
}

// The eight corners of the cube with low-corner voxel (x, y, z), in two steps so that a kernel can issue several cubes' loads before it looks
// at the first: mesh_fetch loads the raw words, mesh_unpack turns them into f32, corner i + 2 j + 4 k at v[...].  x + 1 < nx (likewise y,
// z): a cube's corners are voxels of the volume, so the cell's taps are stored texels, never the clamp's duplicates, and the LINEAR
// indices lie inside the array.
template <int VOL>
struct MeshTaps {
    uint32_t w[is_cell_layout(VOL) ? (VOL == VOL_P8 ? 2 : 4) : 8];  // a cell's words, or the eight texels' bits
};
template <int VOL>
__device__ __forceinline__ void mesh_fetch(const VolumeDesc &V, uint32_t x, uint32_t y, uint32_t z, MeshTaps<VOL> &T) {
    if constexpr (is_cell_layout(VOL)) {
        const char *cptr = reinterpret_cast<const char *>(V.data) + mesh_cell_offset(V, x, y, z);
        if constexpr (VOL == VOL_P8) {
            const uint2 c = *reinterpret_cast<const uint2 *>(cptr);
            T.w[0] = c.x; T.w[1] = c.y;
        } else {
            const uint4 c = *reinterpret_cast<const uint4 *>(cptr);
            T.w[0] = c.x; T.w[1] = c.y; T.w[2] = c.z; T.w[3] = c.w;
        }
    } else {
        const uint64_t row = V.nx, plane = (uint64_t)V.nx * V.ny;
        const uint64_t i0 = (uint64_t)x + row * ((uint64_t)y + (uint64_t)V.ny * (uint64_t)z);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint64_t i = i0 + (b & 1) + ((b >> 1) & 1) * row + (b >> 2) * plane;
            if constexpr (VOL == VOL_LINEAR_U8) T.w[b] = reinterpret_cast<const uint8_t *>(V.data)[i];
            else T.w[b] = reinterpret_cast<const uint16_t *>(V.data)[i];
        }
    }
}
template <int VOL>
__device__ __forceinline__ void mesh_unpack(const MeshTaps<VOL> &T, float (&v)[8]) {
    if constexpr (VOL == VOL_P8) {
#pragma unroll
        for (int b = 0; b < 4; b++) { v[b] = (float)((T.w[0] >> (8 * b)) & 0xffu); v[4 + b] = (float)((T.w[1] >> (8 * b)) & 0xffu); }
    } else if constexpr (is_cell_layout(VOL)) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if constexpr (VOL == VOL_P16) {  // (tap, delta) pairs of f16 that hold u8 values: tap + delta is exact
                const float a = h2f(T.w[k] & 0xffffu), d = h2f(T.w[k] >> 16);
                v[2 * k] = a;
                v[2 * k + 1] = a + d;
            } else {
                v[2 * k] = mesh_texel16<VOL>(T.w[k]);
                v[2 * k + 1] = mesh_texel16<VOL>(T.w[k] >> 16);
            }
        }
    } else {
#pragma unroll
        for (int b = 0; b < 8; b++) v[b] = VOL == VOL_LINEAR_U8 ? (float)T.w[b] : mesh_texel16<VOL>(T.w[b]);
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
    return mesh_cube_inside<VOL == VOL_LINEAR_F16 || VOL == VOL_PF16>(v, D.iso_k);
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
                const uint32_t n = mesh_cube_count(mesh_cube_inside<VOL == VOL_LINEAR_F16 || VOL == VOL_PF16>(v, D.iso_k));
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

static int mesh_fail(vk_ctx *ctx, void *d0, void *d1, int code, const std::string &msg) {
    if (d0) (void)hipFree(d0);
    if (d1) (void)hipFree(d1);
    return fail(ctx, code, msg);
}

template <int VOL>
static void mesh_launch_count(vk_ctx *ctx, uint32_t grid, const VolumeDesc &V, const MeshDesc &D, uint32_t *totals) {
    hipLaunchKernelGGL(mesh_count_kernel<VOL>, dim3(grid), dim3(kMeshThreads), 0, ctx->stream, V, D, totals);
}
template <int VOL>
static void mesh_launch_emit(vk_ctx *ctx, uint32_t grid, const VolumeDesc &V, const MeshDesc &D, const MeshActive *act, uint64_t n_active, float *out, uint64_t cap) {
    hipLaunchKernelGGL(mesh_emit_kernel<VOL>, dim3(grid), dim3(kMeshThreads), 0, ctx->stream, V, D, act, n_active, out, cap);
}
// f(int_tag<VOL>) over the seven volume kinds the pass covers
template <class F>
static void mesh_for_kind(int kind, F &&f) {
    switch (kind) {
        case VOL_P8: f(int_tag<VOL_P8>()); break;
        case VOL_P16: f(int_tag<VOL_P16>()); break;
        case VOL_PF16: f(int_tag<VOL_PF16>()); break;
        case VOL_PU16: f(int_tag<VOL_PU16>()); break;
        case VOL_LINEAR_F16: f(int_tag<VOL_LINEAR_F16>()); break;
        case VOL_LINEAR_U16: f(int_tag<VOL_LINEAR_U16>()); break;
        default: f(int_tag<VOL_LINEAR_U8>()); break;
    }
}

int vk_extract_isosurface(vk_ctx *ctx, const vk_mesh_request *req, const vk_voxel_box *box, float *triangles, uint64_t cap_triangles, uint64_t *n_triangles) {
    if (!ctx) return VK_ERR_INVALID;
    if (const char *why = mesh_validate(req)) return fail(ctx, VK_ERR_INVALID, std::string("vk_extract_isosurface: ") + why);
    if (!n_triangles) return fail(ctx, VK_ERR_INVALID, "vk_extract_isosurface: n_triangles is NULL");
    if (ctx->format < 0) return fail(ctx, VK_ERR_INVALID, "vk_extract_isosurface: no volume uploaded");
    if (box && (req->flags & VK_MESH_CLIP_BOX)) return fail(ctx, VK_ERR_INVALID, "vk_extract_isosurface: VK_MESH_CLIP_BOX takes the box from the clip box: box must be NULL");
    if (box && !hist_box_ok(*box, ctx->nx, ctx->ny, ctx->nz)) return fail(ctx, VK_ERR_INVALID, "vk_extract_isosurface: the box is inverted or leaves the volume");
    if (ctx->format == VK_FMT_RGBA16F_PAIR || !has_table_layout(ctx->vol_kind))
        return fail(ctx, VK_ERR_UNSUPPORTED, "mesh: the pass needs a scalar LINEAR, PACKED or PACKED_PAIRS volume (BRICKED / QUADS / STAGED and RGBA16F_PAIR have no mesh kernels)");
    vk_voxel_box B{0u, 0u, 0u, ctx->nx, ctx->ny, ctx->nz};
    if (box) B = *box;
    else if ((req->flags & VK_MESH_CLIP_BOX) && ctx->clip_on) B = hist_clip_box(ctx->clip_lo, ctx->clip_hi, ctx->nx, ctx->ny, ctx->nz);

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
    VolumeDesc V = ctx->vdesc;
    V.data = ctx->vol; V.data2 = ctx->vol2; V.dist = ctx->dist; V.lut = ctx->lut;
    V.nx = ctx->nx; V.ny = ctx->ny; V.nz = ctx->nz;
    V.nbx = ctx->nbx; V.nby = ctx->nby; V.nbz = ctx->nbz;

    // one work buffer: the header, the list of active chunks, the chunk totals
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t work_bytes = sizeof(MeshScanHeader) + (size_t)D.n_chunks * sizeof(MeshActive) + (size_t)mesh_totals_padded(D.n_chunks) * sizeof(uint32_t);
    void *work = nullptr;
    HIP_TRY(ctx, hipMalloc(&work, work_bytes));
    MeshScanHeader *d_hdr = reinterpret_cast<MeshScanHeader *>(work);
    MeshActive *d_act = reinterpret_cast<MeshActive *>(d_hdr + 1);
    uint32_t *d_totals = reinterpret_cast<uint32_t *>(d_act + D.n_chunks);
    mesh_for_kind(kind, [&](auto vol) { mesh_launch_count<decltype(vol)::value>(ctx, mesh_grid(D.n_chunks, cus, ctx->mesh_max_blocks), V, D, d_totals); });
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kMeshScanThreads), 0, ctx->stream, (const uint32_t *)d_totals, D.n_chunks, d_act, d_hdr);
        e = hipGetLastError();
    }
    MeshScanHeader hdr{};
    if (e == hipSuccess) e = hipMemcpyAsync(&hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return mesh_fail(ctx, work, nullptr, VK_ERR_HIP, std::string("vk_extract_isosurface: ") + hipGetErrorString(e));

    const uint64_t n_write = hdr.n_triangles < cap_triangles ? hdr.n_triangles : cap_triangles;
    if (triangles && n_write) {  // (no triangle to write: no emit launch)
        const size_t out_bytes = (size_t)n_write * 9u * sizeof(float);
        void *d_out = nullptr;
        e = hipMalloc(&d_out, out_bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return mesh_fail(ctx, work, nullptr, e == hipErrorOutOfMemory ? VK_ERR_OOM : VK_ERR_HIP, std::string("vk_extract_isosurface: the output buffer: ") + hipGetErrorString(e));
        }
        mesh_for_kind(kind, [&](auto vol) {
            mesh_launch_emit<decltype(vol)::value>(ctx, mesh_grid(hdr.n_active, cus, ctx->mesh_max_blocks), V, D, d_act, hdr.n_active, reinterpret_cast<float *>(d_out), n_write);
        });
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(triangles, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return mesh_fail(ctx, work, d_out, VK_ERR_HIP, std::string("vk_extract_isosurface: ") + hipGetErrorString(e));
        HIP_TRY(ctx, hipFree(d_out));
    }
    HIP_TRY(ctx, hipFree(work));
    *n_triangles = hdr.n_triangles;
    return VK_OK;
}
