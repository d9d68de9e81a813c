// vk_label_launch.hpp -- what another pass borrows from the label pass's kernels (vk_launch_label.hip): their descriptors and one host
// function per kernel that launches it.  The split pass (vk_launch_split.hip) labels two sets that are no value
// range of the volume -- the eroded markers, the voxels no marker reached -- with the same tile / seam / flatten / scan / number / stats
// kernels: the tile kernel takes its predicate from a word array there, every other kernel reads the parent array alone.
#pragma once

#include "vk_launch.hpp"
#include "vk_label.hpp"

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

// A predicate that comes from a word array: voxel i is foreground iff lo <= w[i] <= hi.  No box: the array holds what the box left.
struct LabelWords {
    const uint32_t *w;
    uint32_t lo, hi;
};

// One launch each, on `stream`; the caller looks at hipGetLastError.  blocks: of the tile grid (tile, seam) or of the chunk grid.
void label_launch_tile_words(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const LabelWords &W, uint32_t *parent);
void label_launch_seam(hipStream_t stream, uint32_t blocks, const LabelDesc &D, uint32_t *parent);
void label_launch_flatten(hipStream_t stream, uint32_t blocks, const LabelDesc &D, uint32_t *parent, uint32_t *chunk_roots, uint32_t *chunk_fg);
void label_launch_scan(hipStream_t stream, uint32_t chunks, uint32_t *chunk_roots, const uint32_t *chunk_fg, unsigned long long *totals);
void label_launch_number(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const uint32_t *parent, const uint32_t *chunk_offset, uint32_t *labels, const LabelRecords &R);
void label_launch_stats(hipStream_t stream, uint32_t blocks, const LabelDesc &D, const uint32_t *parent, uint32_t *labels, const LabelRecords &R);
