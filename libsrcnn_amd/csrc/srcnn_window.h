// srcnn_window.h -- internal interface of the window kernels (srcnn_window.hip) behind the rect call.  Not installed; the
// public surface is include/srcnn_amd_rect.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "srcnn_kernels.h"

namespace srcnn {

// Horizontal pass for destination columns [c0, c0 + nc) only: dst is tight (nc floats per row), row y of it is made from row y
// of src (src_stride floats per row), whose column 0 is source column src_col_base.  The arithmetic of k_resample_rows.
void launch_window_rows(const float* src, size_t src_stride, int src_col_base, float* dst, int c0, int nc, int rows,
                        const DevAxisTable& t, hipStream_t s);
// Vertical pass for destination rows [r0, r0 + rows) of nc columns: dst is tight (row r0 at offset 0), src has src_stride floats
// per row, its row 0 is source row src_row_base and its column 0 the window's first column.  The arithmetic of k_resample_cols.
void launch_window_cols(const float* src, size_t src_stride, int src_row_base, float* dst, int nc, int r0, int rows,
                        const DevAxisTable& t, hipStream_t s);
// w x rows floats from src (src_stride floats per row) to dst (dst_stride floats per row): 16-byte stores where dst and its
// stride allow, single floats for the rest of each row.  Nothing outside the w floats of a destination row is written.
void launch_window_copy(const float* src, size_t src_stride, float* dst, size_t dst_stride, int w, int rows, hipStream_t s);

}  // namespace srcnn
