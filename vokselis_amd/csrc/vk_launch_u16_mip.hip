// vk_launch_u16_mip.hip -- the cell march on R16_UNORM volumes under the maximum-intensity projection: raymarch_u16_kernel (vk_march_u16.hpp) for
// U16_MIP, LINEAR and PACKED, every variant.
#include "vk_march_u16.hpp"

using namespace vk;

void launch_u16_mip(vk_ctx *ctx, const LaunchDesc &L, const VolumeDesc &V, const TfDesc &T, const LightDesc &Li, const IsoDesc &I, const ClipDesc *Cl, uint32_t grid, bool count,
                   bool skip, bool safe) {
    launch_u16_family<U16_MIP>(ctx, L, V, T, Li, I, Cl, grid, count, skip, safe);
}
