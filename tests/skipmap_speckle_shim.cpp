// The library's lone-speckle encoder (vk_tf.hpp: speckle_code) behind a C entry point, for tests/np_skipmap_reference.py: the skip-map
// tests check WHERE the maps carry a code, and take the code's value from here.  Plain g++, loaded with ctypes.
#include <stdint.h>

#include "vk_tf.hpp"

extern "C" void skm_speckle_codes(const float *taps, uint64_t n_cells, uint8_t *out) {  // taps: [n_cells][8], tap b = dx | dy << 1 | dz << 2
    for (uint64_t c = 0; c < n_cells; c++) out[c] = (uint8_t)vk::speckle_code(taps + 8 * c);
}
