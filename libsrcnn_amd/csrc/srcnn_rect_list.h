// srcnn_rect_list.h -- launchers of the rect list call's kernels (srcnn_rect_list.hip), for srcnn_capi.cpp.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "srcnn_kernels.h"
#include "srcnn_rect_atlas.hpp"

namespace srcnn {

// d: the device copy of a pass's descriptor table (ncells + 1 entries, build_cell_descs); `end`: its closing entry (the totals).
// atlas_w: floats per row of the atlas planes.
void launch_list_resample(const float* d_in, size_t in_stride, unsigned w, unsigned h, const DevAxisTable& th, const DevAxisTable& tv,
                          const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas, unsigned atlas_w, hipStream_t s);
// out-of-plane samples within `depth` of the rect, in `planes` planes `plane_stride` floats apart
void launch_list_replicate(const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas, unsigned atlas_w, size_t plane_stride,
                           unsigned planes, unsigned depth, hipStream_t s);
void launch_list_scatter(const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, const float* atlas, unsigned atlas_w, hipStream_t s);

}  // namespace srcnn
