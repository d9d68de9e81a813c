// vk_dist_launch.hpp -- what another pass borrows from the distance pass's kernels (vk_launch_dist.hip): one round of the transform to
// the complement of a value range, left on the device.  The split pass (vk_launch_split.hip) erodes with it.
#pragma once

#include "vk_launch.hpp"
#include "vk_dist.hpp"

// D2(not S, .) over the integer `spacing` into a[0 .. n): the column, line y and line x kernels of vk_distance_transform(VK_DIST_INSIDE),
// unchanged, through the same launch functions and grids (dist_max_blocks and dist_x_plain hold), on the context's stream.  S: the stored texels in [lo_k, hi_k] (the kernel's scale) inside B.  b and stack: n words each,
// scratch.  The caller has checked what vk_distance_transform checks (a scalar kind, the voxel count, dist_d2_fits) and looks at
// hipGetLastError.
void dist_launch_inside(vk_ctx *ctx, const vk_voxel_box &B, float lo_k, float hi_k, const uint32_t spacing[3], uint32_t *a, uint32_t *b, uint32_t *stack);
