// The status words of the single-pass scans' decoupled look-back (preprocess.hip: ds_segments_body; cloud_crop.hip: crop_cloud_kernel),
// stated once.  One word per tile: {epoch : 30, state : 2, value : 32}; state kLookAgg: value is the tile's own total, kLookPrefix: the
// inclusive prefix over the tiles 0 .. this one.  Words of earlier launches carry an older epoch and read as "nothing yet": nothing is
// ever cleared.  (The look-back loop itself stays written in both kernels: sharing it moved crop_cloud_kernel's register row,
// profiles/cloud_ops_kernel_resources.txt.)
#pragma once
#include "common.hpp"

namespace sga {

constexpr int kLookEpochShift = 34;
constexpr unsigned long long kLookAgg = 1ull << 32, kLookPrefix = 2ull << 32;
// preprocess.hip: the context's status words (ctx->vg_status; grow-only) with room for a launch of `tiles` workgroups, and its epoch
int voxelgrid_status(sga_context* ctx, uint32_t tiles, unsigned* epoch);

}  // namespace sga
