// vk_label_launch.hpp -- what another pass borrows from the label pass's kernels (vk_launch_label.hip): their descriptors and one host
// function per kernel that launches it.  The split pass (vk_launch_split.hip) labels two sets that are no value
// range of the volume -- the eroded markers, the voxels no marker reached -- with the same tile / seam / flatten / scan / number / stats
// kernels: the tile kernel takes its predicate from a word array there, every other kernel reads the parent array alone.
#pragma once

#include "vk_launch.hpp"
#include "vk_label.hpp"

#include <vector>

struct LabelDesc {
    uint32_t nx, ny, nz, conn_sum;
    vk_voxel_box box;
    uint32_t ntx, nty;
    uint64_t tiles;
    uint64_t n;  // voxels
    uint32_t chunks;
    float lo_k, hi_k;
    uint32_t fill_bits, invert, pad;
};

// A component's record on the device: what the label kernel gathers into.
struct LabelRecords {
    uint32_t *first, *size, *box;  // box: 6 words per component -- the smallest x, y, z, then the largest
};

// The first n_rec records into `components`, the call's last download: the arrays' copies, the call's last wait, then the records, a box's
// upper corner made exclusive.  sizes: the host's copy of R.size where the caller holds one (it is not downloaded again), else NULL.
inline int label_download_components(vk::PassCall &call, const LabelRecords &R, const uint32_t *sizes, uint64_t n_rec, vk_component *components) {
    std::vector<uint32_t> firsts((size_t)n_rec), own(sizes ? (size_t)0u : (size_t)n_rec), boxes((size_t)n_rec * 6u);
    if (n_rec) {
        call.download(firsts.data(), R.first, (size_t)n_rec * 4u);
        if (!sizes) call.download(own.data(), R.size, (size_t)n_rec * 4u);
        call.download(boxes.data(), R.box, (size_t)n_rec * 24u);
    }
    if (int rc = call.finish()) return rc;
    if (!sizes) sizes = own.data();
    for (uint64_t c = 0; c < n_rec; c++) {
        const uint32_t *b = boxes.data() + 6u * c;
        components[c].n_voxels = sizes[c];
        components[c].first = firsts[c];
        components[c].box = vk_voxel_box{b[0], b[1], b[2], b[3] + 1u, b[4] + 1u, b[5] + 1u};
    }
    return VK_OK;
}

// A predicate that comes from a word array: voxel i is foreground iff lo <= w[i] <= hi.  No box: the array holds what the box left.
struct LabelWords {
    const uint32_t *w;
    uint32_t lo, hi;
};

// One launch each, on `stream`; the caller looks at hipGetLastError.  blocks: of the tile grid (tile, seam) or of the chunk grid.
// kind: the volume's scalar kind (with_scalar_kind): the predicate is the volume's stored texel against [D.lo_k, D.hi_k] inside D.box
void label_launch_tile(hipStream_t stream, uint32_t blocks, int kind, const vk::VolumeDesc &V, const LabelDesc &D, uint32_t *parent);
void label_launch_tile_words(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const LabelWords &W, uint32_t *parent);
void label_launch_seam(hipStream_t stream, uint32_t blocks, const LabelDesc &D, uint32_t *parent);
void label_launch_flatten(hipStream_t stream, uint32_t blocks, const LabelDesc &D, uint32_t *parent, uint32_t *chunk_roots, uint32_t *chunk_fg);
void label_launch_scan(hipStream_t stream, uint32_t chunks, uint32_t *chunk_roots, const uint32_t *chunk_fg, unsigned long long *totals);
void label_launch_number(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const uint32_t *parent, const uint32_t *chunk_offset, uint32_t *labels, const LabelRecords &R);
void label_launch_stats(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const uint32_t *parent, uint32_t *labels, const LabelRecords &R);
