// srcnn_delta.h -- launcher of the delta call's kernel (srcnn_delta.hip), for srcnn_delta_call.cpp.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

namespace srcnn {

// Clears the cols x rows flag bytes at d_flags, then sets to 1 the flag of every tile whose source rectangle holds a sample
// with different bits in d_prev and d_cur (w x h floats, pitches in bytes, multiples of 4).  d_spans: the table image of
// delta_span_image (srcnn_delta.hpp), 2 * (cols + rows) words, both axes monotone; cols, rows <= kDeltaMaxAxisTiles.
// Asynchronous on s.  After it every one of the cols * rows bytes has been written and no byte outside has.
void launch_delta_flags(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h,
                        const unsigned* d_spans, unsigned cols, unsigned rows, unsigned char* d_flags, hipStream_t s);

}  // namespace srcnn
