// vk_pass_blocks.hpp -- the device blocks the value-range passes share: a reduction over a wave, a sum over a
// workgroup, a workgroup's row of partial totals, the store of a gained value.  tile_coords is vk_box.hpp's, with the host programs; the
// host half (PassPartials, PassCall::iterate) is vk_launch.hpp's.  Plain inlined functions, held to the ISA by tools/isa_diff.py.
#pragma once

#include "vk_common.hpp"
#include "vk_label.hpp"

namespace vk {

// op over the v (uint32_t or unsigned long long) of a wave's lanes, in lane 0.  log2(warpSize) shuffles in which every lane takes part:
// the call stands where the wave's control flow is uniform.
struct WaveMin { template <class T> __device__ __forceinline__ T operator()(T v, T o) const { return o < v ? o : v; } };
struct WaveMax { template <class T> __device__ __forceinline__ T operator()(T v, T o) const { return o > v ? o : v; } };
struct WaveOr { template <class T> __device__ __forceinline__ T operator()(T v, T o) const { return v | o; } };
struct WaveAdd { template <class T> __device__ __forceinline__ T operator()(T v, T o) const { return v + o; } };
template <class T, class OP>
__device__ __forceinline__ T wave_reduce(T v, OP op) {
    for (int d = warpSize / 2; d > 0; d >>= 1) v = op(v, (T)__shfl_down(v, d));
    return v;
}

// the sum of v (either type) over a workgroup's threads, added to *slot (LDS, zeroed before): lanes are combined in registers, one LDS
// add per wave
template <class T>
__device__ __forceinline__ void block_add(unsigned long long *slot, T v) {
    const unsigned long long s = wave_reduce((unsigned long long)v, WaveAdd());
    if ((threadIdx.x & (warpSize - 1)) == 0 && s) atomicAdd(slot, s);
}

// Partial totals per workgroup: a kernel zeroes s_n in LDS, accumulates into it and publishes it as row blockIdx.x of `partial`, ROW
// words a row, which the host adds up (vk_launch.hpp: PassPartials).  The publishing: the barrier behind the accumulation, then the first
// W words.  Every thread of the workgroup comes here: the call stands outside every branch and loop that is not block-uniform.  A kernel
// whose row holds more than sums writes its other words itself.
template <uint32_t ROW, uint32_t W = ROW>
__device__ __forceinline__ void publish_partials(unsigned long long *__restrict__ partial, const unsigned long long *s_n) {
    __syncthreads();
    if (threadIdx.x < W) partial[(size_t)ROW * blockIdx.x + threadIdx.x] = s_n[threadIdx.x];
}

// F of a value that a call's gain has scaled, as label_fill_bits forms it, for a dense array of class CLASS
template <int CLASS>
__device__ __forceinline__ uint32_t store_gained_bits(float v) {
    if constexpr (CLASS == TEXEL_U8) return filter_store_unorm(v * 255.0f, 255.0f);
    else if constexpr (CLASS == TEXEL_U16) return filter_store_unorm(v * 65535.0f, 65535.0f);
    else return filter_store_f16(v);
}

}  // namespace vk
