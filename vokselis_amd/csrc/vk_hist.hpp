// vk_hist.hpp -- the volume histogram and region statistics (vk_volume_histogram, vk_histogram_window): the validation of
// a caller's vk_histogram (which forms lo_k, hi_k, k1, k2), the classification of one texel, the order-preserving key of min and max, the
// window of two percentiles, and the grid and flush arithmetic of the kernels (the box rules: vk_box.hpp), shared by the kernels and
// their host (vk_launch_hist.hip) and the host fuzz (tests/hist_fuzz.cpp, plain g++ under ASan / UBSan).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vokselis_hip.h"
#include "vk_box.hpp"
#include "vk_tf.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VK_HIST_HD __host__ __device__ __forceinline__
#else
#define VK_HIST_HD inline
#endif

namespace vk {

// The constants of a request on the kernel's scale
struct HistConsts {
    float lo_k, hi_k, k1, k2;
    uint32_t bins;
};

// A caller's request into the constants.  Returns nullptr, or what is wrong (VK_ERR_INVALID).
inline const char *hist_validate(const vk_histogram *h, SampleScale scale, HistConsts &K) {
    if (!h) return "the request is NULL";
    if (h->bins < 1u || h->bins > (uint32_t)VK_HIST_MAX_BINS) return "bins must be in [1, VK_HIST_MAX_BINS]";
    if (!isfinite(h->lo) || !isfinite(h->hi) || !(h->hi > h->lo)) return "lo and hi must be finite, lo < hi";
    if (h->flags & ~(uint32_t)VK_HIST_CLIP_BOX) return "unknown flag (VK_HIST_CLIP_BOX)";
    const double S = sample_scale(scale), lo = (double)h->lo, span = (double)h->hi - (double)h->lo, bins = (double)h->bins;
    K.lo_k = (float)(lo * S);
    K.hi_k = (float)((double)h->hi * S);
    K.k1 = (float)(bins / (span * S));
    K.k2 = (float)(-lo * bins / span);
    K.bins = h->bins;
    return nullptr;
}

// Where a texel goes: its bin, or one of the three categories.  The comparisons are made on floats before the conversion: a k1 that
// overflowed (a domain a few denormals wide) gives u = NaN or inf, which land in bin 0 or the top bin, never in an undefined conversion.
enum : int { HIST_NAN = -1, HIST_BELOW = -2, HIST_ABOVE = -3 };
VK_HIST_HD int hist_bin(float t, float lo_k, float hi_k, float k1, float k2, uint32_t bins) {
    if (t != t) return HIST_NAN;
    if (t < lo_k) return HIST_BELOW;
    if (t > hi_k) return HIST_ABOVE;
    const float u = floorf(fmaf(t, k1, k2));
    if (!(u >= 1.0f)) return 0;
    return u >= (float)bins ? (int)bins - 1 : (int)u;  // (bins <= 4096: exact as a float)
}
// the slot of a classification in an array of bins + 3 counters: the bins, then NaN, below, above
VK_HIST_HD uint32_t hist_slot(int b, uint32_t bins) { return b >= 0 ? (uint32_t)b : bins + (uint32_t)(-1 - b); }
constexpr uint32_t kHistCats = 3;

// The order-preserving key of an f32: a < b implies key(a) < key(b) for all non-NaN a, b; -0 lies below +0.  A key of 0 and a key of
// 0xffffffff belong to NaNs only, which never enter: both serve as "nothing seen" (the device keeps the maximum of key and of ~key in a
// pair of words that start at 0).
VK_HIST_HD uint32_t hist_key(float f) {
    uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
    b = __float_as_uint(f);
#else
    memcpy(&b, &f, 4);
#endif
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float hist_key_value(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &b, 4);
    return f;
}
// the two words the device leaves -- max over ~key, max over key -- into min and max
inline void hist_minmax_decode(uint32_t inv_min, uint32_t max_key, float &mn, float &mx) {
    mn = inv_min == 0u ? INFINITY : hist_key_value(~inv_min);
    mx = max_key == 0u ? -INFINITY : hist_key_value(max_key);
}

// The window of two percentiles (vk_histogram_window).  Returns nullptr, or what is wrong.
inline const char *hist_window(const uint64_t *counts, uint32_t bins, float lo, float hi, double p_lo, double p_hi, float &w_lo, float &w_hi) {
    if (!counts) return "counts is NULL";
    if (bins < 1u || bins > (uint32_t)VK_HIST_MAX_BINS) return "bins must be in [1, VK_HIST_MAX_BINS]";
    if (!isfinite(lo) || !isfinite(hi) || !(hi > lo)) return "lo and hi must be finite, lo < hi";
    if (!(0.0 <= p_lo && p_lo < p_hi && p_hi <= 1.0)) return "needs 0 <= p_lo < p_hi <= 1";
    uint64_t N = 0;
    for (uint32_t i = 0; i < bins; i++) N += counts[i];
    if (N == 0u) return "the histogram is empty";
    const double r_lo = floor(p_lo * (double)N);
    double r_hi = ceil(p_hi * (double)N);
    if (r_hi > (double)N) r_hi = (double)N;
    uint32_t b_lo = bins - 1u, b_hi = bins - 1u;
    uint64_t run = 0;
    bool have_lo = false;
    for (uint32_t i = 0; i < bins; i++) {
        run += counts[i];
        if (!have_lo && (double)run > r_lo) { b_lo = i; have_lo = true; }
        if ((double)run >= r_hi) { b_hi = i; break; }
    }
    if (b_hi < b_lo) b_hi = b_lo;
    const double span = (double)hi - (double)lo;
    const float a = (float)((double)lo + (double)b_lo * span / (double)bins), b = (float)((double)lo + ((double)b_hi + 1.0) * span / (double)bins);
    if (!(a < b)) return "the window is empty once rounded to f32";
    w_lo = a;
    w_hi = b;
    return nullptr;
}

// ---- the kernels' launch arithmetic ---------------------------------------------------------------------------------------------
constexpr uint32_t kHistThreads = 256;       // a workgroup: four waves
constexpr uint32_t kHistBlocksPerCU = 8;     // 16 KiB of LDS and four waves each: a CU holds eight
constexpr uint32_t kHistLinearChunk = 16;    // LINEAR: bytes a lane loads at a time
constexpr uint32_t kHistWaveCells = 64;      // cell layouts: a wave reads 8 bricks x 8 even cells, one cell per lane
constexpr uint64_t kHistFlushVoxels = 0xffffffffull;  // a workgroup merges before its u32 counters could have counted more

// blocks of a launch: enough for the work (a block takes `per_block` items per pass of its grid-stride loop), at most what the device
// holds at once, at most the debug cap (0: none), at least 1
VK_HIST_HD uint32_t hist_grid(uint64_t items, uint32_t per_block, uint32_t cus, uint32_t max_blocks) {
    uint64_t g = (items + per_block - 1u) / per_block;
    const uint64_t full = (uint64_t)(cus ? cus : 1u) * kHistBlocksPerCU;
    g = g > full ? full : g;
    if (max_blocks && g > max_blocks) g = max_blocks;
    return g < 1u ? 1u : (uint32_t)g;
}
// passes of the grid-stride loop a workgroup may count into its u32 counters before it merges: every pass counts at most
// voxels_per_pass, so the passes' total stays within kHistFlushVoxels
VK_HIST_HD uint32_t hist_flush_passes(uint32_t voxels_per_pass) {
    const uint64_t p = kHistFlushVoxels / (uint64_t)voxels_per_pass;
    return p > 0xffffffffull ? 0xffffffffu : (uint32_t)p;
}
// voxels a workgroup counts per pass at most: LINEAR, a chunk per lane of `elem` bytes a voxel; cells, eight taps per lane
VK_HIST_HD uint32_t hist_pass_voxels_linear(uint32_t elem) { return kHistThreads * (kHistLinearChunk / elem); }
VK_HIST_HD uint32_t hist_pass_voxels_cells() { return kHistThreads * 8u; }

// LINEAR: the box as runs of contiguous voxels.  Run (a, b), a < na, b < nb, starts at voxel off0 + a sa + b sb and is `len` voxels
// long; full rows merge into their plane, full planes into one run.
struct HistRuns {
    uint64_t off0, len, sa, sb;
    uint32_t na, nb;
};
inline HistRuns hist_runs(const vk_voxel_box &b, uint32_t nx, uint32_t ny) {
    HistRuns R;
    R.off0 = voxel_index(b.x0, b.y0, b.z0, nx, ny);
    R.len = b.x1 - b.x0; R.na = b.y1 - b.y0; R.sa = nx; R.nb = b.z1 - b.z0; R.sb = (uint64_t)nx * ny;
    for (int k = 0; k < 2; k++)
        if (R.na == 1u || R.len == R.sa) { R.len *= R.na; R.na = R.nb; R.sa = R.sb; R.nb = 1u; }
    return R;
}
// 16-byte chunks a run of `len` voxels of `elem` bytes can touch at most, whatever its alignment
VK_HIST_HD uint64_t hist_run_chunks(uint64_t len, uint32_t elem) { return (len * elem + kHistLinearChunk - 1u) / kHistLinearChunk + 1u; }

// Cell layouts: the even cells of the box in bricks.  Even cell j (low-corner voxel 2 j) of an axis covers voxels 2 j and 2 j + 1; the box
// [x0, x1) needs cells [x0 >> 1, (x1 + 1) >> 1), which lie two to a brick: bricks [j0 >> 1, (j1 + 1) >> 1).
VK_HIST_HD void hist_cell_range(uint32_t x0, uint32_t x1, uint32_t &b0, uint32_t &nb) {
    const uint32_t j0 = x0 >> 1, j1 = (x1 + 1u) >> 1;
    b0 = j0 >> 1;
    nb = x1 > x0 ? ((j1 + 1u) >> 1) - b0 : 0u;
}

}  // namespace vk
