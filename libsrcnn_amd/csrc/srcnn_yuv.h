// srcnn_yuv.h -- internal interface of the 8-bit YUV 4:2:0 conversion kernels (srcnn_yuv.hip).  Not installed; the public
// surface is include/srcnn_amd_yuv.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace srcnn {

// Pitched u8 plane -> tight float plane(s).  nv12 = false: `w` samples per row -> d0.  nv12 = true: `w` interleaved
// (U, V) pairs per row -> d0 (U) and d1 (V).  Rows [0, rows).
void launch_yuv_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, bool nv12, float* d0, float* d1,
                       hipStream_t s);
// Tight float rows -> pitched u8 plane, rows [0, rows) of the source to destination rows [row0, row0 + rows).
// sat = false: (unsigned char) v (Y': layer 3 already clamps); sat = true: MIN(255), MAX(0), truncation (chroma).
// s1 != NULL: NV12, `w` pairs (s0[i], s1[i]) interleaved per row.
void launch_yuv_pack(const float* s0, const float* s1, unsigned w, unsigned rows, bool sat, unsigned char* dst, size_t pitch,
                     unsigned row0, hipStream_t s);

}  // namespace srcnn
