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

// Two integer pixel surfaces of up to four planes that share one pixel grid (an RGB(A) image of include/srcnn_amd_rgb.h), as
// k_delta_flags_bytes compares them: passed by value.
struct DeltaBytePlanes {
    const unsigned char* prev[4];
    const unsigned char* cur[4];
    size_t prev_pitch[4], cur_pitch[4];  // bytes, at least row_bytes
    unsigned planes;                     // 1 ... 4
    unsigned row_bytes;                  // bytes of one row of one plane: bpp * w
    unsigned rows;                       // h
    unsigned bpp;                        // bytes of one pixel in a plane's row: 3, 4, 6, 8 interleaved, 1 or 2 planar
};

// The same for byte surfaces (include/srcnn_amd_rgb_delta.h): clears the cols x rows flag bytes, then sets to 1 the flag of every
// tile whose source rectangle (d_spans: the image of the RGB(A) grid's tables, in PIXELS) holds a pixel with a differing byte in
// any plane.  Bases and pitches need no alignment; nothing past a row's row_bytes is read.  row_bytes < 2^30, row_bytes * rows < 2^34.
void launch_delta_flags_bytes(const DeltaBytePlanes& p, const unsigned* d_spans, unsigned cols, unsigned rows, unsigned char* d_flags, hipStream_t s);

}  // namespace srcnn
