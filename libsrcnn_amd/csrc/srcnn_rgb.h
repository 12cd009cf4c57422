// srcnn_rgb.h -- internal interface of the RGB(A) conversion kernels (srcnn_rgb.hip).  Not installed; the public surface is
// include/srcnn_amd_rgb.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "srcnn_frame_rules.h"

namespace srcnn {

// Pitched integer plane(s) -> tight float planes out[0..3] = Y, Cb, Cr, A (w floats per row; out[3] only with alpha), rows
// [0, rows), with the split arithmetic of k_rgb_split.  Interleaved: src[0] only.  At bps == 2 bases and pitches are even.
void launch_rgb_unpack(const RgbRule& f, const unsigned char* const src[4], const size_t pitch[4], unsigned w, unsigned rows,
                       float* const out[4], hipStream_t s);
// Tight float rows in[0..3] = Y', Cb', Cr', A' (row 0 of each = destination row row0) -> destination rows [row0, row0 + rows)
// of the pitched integer plane(s), with the merge arithmetic of k_ycc_merge; conv != NULL: (unsigned)(Y' * f.up) as well, one
// sample of f.bps bytes per pixel.
void launch_rgb_pack(const RgbRule& f, const float* const in[4], unsigned w, unsigned rows, unsigned char* const dst[4],
                     const size_t pitch[4], unsigned row0, unsigned char* conv, size_t conv_pitch, hipStream_t s);

}  // namespace srcnn
