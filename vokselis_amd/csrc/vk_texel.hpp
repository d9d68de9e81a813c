// vk_texel.hpp -- the stored texels of the scalar LINEAR, PACKED and PACKED_PAIRS kinds, read by voxel index: where a cell is, its load,
// tap b of it as stored bits or as f32, a LINEAR element, the decode of a 16-bit texel.  For the passes that are not a ray (histogram,
// mesh extraction, filter); the marches share the cell load (vk_march_parts.hpp includes this header) and keep their own 32-bit address
// arithmetic.  Plain inlined functions: tools/isa_diff.py holds every change here to the parent's device code.
#pragma once

#include "vk_box.hpp"
#include "vk_common.hpp"

namespace vk {

// ---- a cell ---------------------------------------------------------------------------------------------------------------------
template <int VOL>
struct CellBits { u32x4_t v; };
template <>
struct CellBits<VOL_P8> { u32x2_t v; };

// the byte offset of the cell with low-corner voxel (ix, iy, iz) (vk_common.hpp: VolumeDesc), held inside the cell array
// (the marches' twin on int indices in 32-bit arithmetic: vk_march_parts.hpp, safe_cell_offset)
__device__ __forceinline__ int64_t cell_offset(const VolumeDesc &V, uint32_t ix, uint32_t iy, uint32_t iz) {
    const int64_t off = (int64_t)(iz >> 2) * V.kz + (int64_t)(iy >> 2) * (int64_t)V.ky + (int64_t)(ix >> 2) * (int64_t)V.kx +
                        (((int64_t)iz << V.sh_z) + ((int64_t)iy << V.sh_y) + ((int64_t)ix << V.sh_x)) + V.c0;
    return off < 0 ? 0 : (off > V.max_off ? V.max_off : off);
}
__device__ __forceinline__ const char *cell_ptr(const VolumeDesc &V, uint32_t ix, uint32_t iy, uint32_t iz) {
    return reinterpret_cast<const char *>(V.data) + cell_offset(V, ix, iy, iz);
}
// the cell at a pointer: its 2 or 4 words
template <int VOL>
__device__ __forceinline__ CellBits<VOL> load_cell(const char *cptr) {
    CellBits<VOL> cb;
    if constexpr (VOL == VOL_P8) { const uint2 c = *reinterpret_cast<const uint2 *>(cptr); cb.v.x = c.x; cb.v.y = c.y; }
    else { const uint4 c = *reinterpret_cast<const uint4 *>(cptr); cb.v.x = c.x; cb.v.y = c.y; cb.v.z = c.z; cb.v.w = c.w; }
    return cb;
}
// ... as an array of words
constexpr int cell_words(int VOL) { return VOL == VOL_P8 ? 2 : 4; }
template <int VOL>
__device__ __forceinline__ void load_cell(const char *cptr, uint32_t (&w)[cell_words(VOL)]) {
    const CellBits<VOL> c = load_cell<VOL>(cptr);
#pragma unroll
    for (int k = 0; k < cell_words(VOL); k++) w[k] = c.v[k];
}

// ---- a texel --------------------------------------------------------------------------------------------------------------------
// element e of words that hold 8-bit or 16-bit texels (an array or a vector of u32)
template <int BITS, class W>
__device__ __forceinline__ uint32_t texel_field(const W &w, uint32_t e) {
    if constexpr (BITS == 8) return (w[e >> 2] >> (8u * (e & 3u))) & 0xffu;
    else return (w[e >> 1] >> (16u * (e & 1u))) & 0xffffu;
}
// a stored texel (its bits, nothing above them) as f32 on the kernel's scale: the half's value, or the integer
template <int VOL>
__device__ __forceinline__ float texel_f32(uint32_t bits) {
    if constexpr (is_f16_kind(VOL)) return h2f(bits);
    else return (float)bits;
}
// PACKED_PAIRS: a word is a (tap, delta) pair of f16 that hold u8 values: tap + delta is exact.  The even tap, or the odd one.
__device__ __forceinline__ float pair_tap(uint32_t word, bool odd) {
    const float a = h2f(word & 0xffffu), d = h2f(word >> 16);
    return odd ? a + d : a;
}

// Tap b of a loaded cell's words w (an array, or CellBits::v), b = dx + 2 dy + 4 dz: as stored bits (the u8 or u16 value, or the
// half; PACKED_PAIRS: the sum, converted), or as f32.  Two entry points side by side: the bits are the histogram's, the f32 the mesh's,
// and PACKED_PAIRS reaches neither through the other.
template <int VOL, class W>
__device__ __forceinline__ uint32_t cell_tap_bits(const W &w, uint32_t b) {
    if constexpr (VOL == VOL_P8) return texel_field<8>(w, b);
    else if constexpr (VOL == VOL_P16) return (uint32_t)pair_tap(w[b >> 1], (b & 1u) != 0u);
    else return texel_field<16>(w, b);
}
template <int VOL, class W>
__device__ __forceinline__ float cell_tap_f32(const W &w, uint32_t b) {
    if constexpr (VOL == VOL_P16) return pair_tap(w[b >> 1], (b & 1u) != 0u);
    else return texel_f32<VOL>(cell_tap_bits<VOL>(w, b));
}

// element i of a LINEAR array, as stored bits
template <int VOL>
__device__ __forceinline__ uint32_t linear_texel_bits(const void *data, uint64_t i) {
    if constexpr (VOL == VOL_LINEAR_U8) return reinterpret_cast<const uint8_t *>(data)[i];
    else return reinterpret_cast<const uint16_t *>(data)[i];
}

// The stored texel of voxel (x, y, z), x < nx (likewise y, z), as its bits, by a load of its own.  Cell layouts: tap
// (x & 1) + 2 (y & 1) + 4 (z & 1) of the cell whose low corner is the voxel with its low bits cleared -- a voxel of the volume, so the
// cell exists and the tap is a stored texel, not one of the clamp's duplicates; only the tap's byte, half or pair is loaded.
template <int VOL>
__device__ __forceinline__ uint32_t voxel_texel_bits(const VolumeDesc &V, uint32_t x, uint32_t y, uint32_t z) {
    if constexpr (is_cell_layout(VOL)) {
        const char *cptr = cell_ptr(V, x & ~1u, y & ~1u, z & ~1u);
        const uint32_t b = (x & 1u) | ((y & 1u) << 1) | ((z & 1u) << 2);
        if constexpr (VOL == VOL_P8) return reinterpret_cast<const uint8_t *>(cptr)[b];
        else if constexpr (VOL == VOL_P16) return (uint32_t)pair_tap(reinterpret_cast<const uint32_t *>(cptr)[b >> 1], (b & 1u) != 0u);
        else return reinterpret_cast<const uint16_t *>(cptr)[b];
    } else return linear_texel_bits<VOL>(V.data, voxel_index(x, y, z, V.nx, V.ny));
}

// bits as texel i of a dense array of class CLASS (texel_class): a u8, or a u16 / half
template <int CLASS>
__device__ __forceinline__ void store_texel_bits(void *__restrict__ out, uint64_t i, uint32_t bits) {
    if constexpr (CLASS == TEXEL_U8) reinterpret_cast<uint8_t *>(out)[i] = (uint8_t)bits;
    else reinterpret_cast<uint16_t *>(out)[i] = (uint16_t)bits;
}

}  // namespace vk
