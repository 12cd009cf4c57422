// srcnn_rgb.h -- internal interface of the RGB(A) conversion kernels (srcnn_rgb.hip).  Not installed; the public surface is
// include/srcnn_amd_rgb.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "srcnn_frame_rules.h"
#include "srcnn_kernels.h"

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

// ---- the window forms behind the rect call (srcnn_rgb_window.hip; include/srcnn_amd_rgb_rect.h) ----
// Samples [sx0, sx0 + sw) x [sy0, sy0 + sh) of the pitched integer plane(s) src (the WHOLE image) -> a tight sw x sh float Y
// window, with the Y line of launch_rgb_unpack.  No byte outside that rectangle is read.
void launch_rgb_window_y(const RgbRule& f, const unsigned char* const src[4], const size_t pitch[4], unsigned sx0, unsigned sy0,
                         unsigned sw, unsigned sh, float* y, hipStream_t s);
// One band of the rect: Cb', Cr' (and A') of output columns [x0, x0 + rw) and rows [gy0, gy0 + rows) resampled from the whole
// w x h integer source with the tables th (columns) and tv (rows), an up-scale in both axes, merged with yband (tight, rw floats
// per row) as launch_rgb_pack merges, into rows [row0, row0 + rows) of dst (whose first pixel is the rect's) and of conv.  The
// caller has asked window_tile_fits (srcnn_window_tile.h) for that range.
void launch_rgb_window_merge(const RgbRule& f, const unsigned char* const src[4], const size_t spitch[4], unsigned w, unsigned h,
                             const float* yband, unsigned x0, unsigned gy0, unsigned rw, unsigned rows,
                             const DevAxisTable& th, const DevAxisTable& tv, unsigned char* const dst[4], const size_t dpitch[4],
                             unsigned row0, unsigned char* conv, size_t conv_pitch, hipStream_t s);

// ---- the two colour kernels of the rect LIST call (srcnn_rgb_rect_list.hip; include/srcnn_amd_rgb_rect_list.h) ----
struct ListCellDesc;         // srcnn_rect_atlas.hpp
struct ListDstDesc;          // srcnn_rgb_rect_atlas.hpp
// launch_list_resample (srcnn_rect_list.h) reading Y off the pitched integer plane(s) src (the WHOLE image) with the Y line of
// launch_rgb_window_y.  th, tv: the Y tables.
void launch_rgb_list_resample(const RgbRule& f, const unsigned char* const src[4], const size_t spitch[4], unsigned w, unsigned h,
                              const DevAxisTable& th, const DevAxisTable& tv, const ListCellDesc* d, unsigned ncells, const ListCellDesc& end,
                              float* atlas, unsigned atlas_w, hipStream_t s);
// Every rect of a pass: Cb', Cr' (and A') resampled from src with the chroma tables cth (columns) and ctv (rows) as
// launch_rgb_window_merge resamples them, merged with Y' of the atlas result and stored where dd (the device copy of the
// pass's destination table, entry k for cell k) points.  The router has asked window_tile_fits for every rect.
void launch_rgb_list_merge(const RgbRule& f, const unsigned char* const src[4], const size_t spitch[4], unsigned w, unsigned h,
                           const DevAxisTable& cth, const DevAxisTable& ctv, const ListCellDesc* d, const ListDstDesc* dd, unsigned ncells,
                           const ListCellDesc& end, const float* atlas, unsigned atlas_w, hipStream_t s);

}  // namespace srcnn

// One launch of the <BPS, PLANAR, D> instance of an RGB kernel template that the rule f selects (blocks of 256 threads)
#define RGB_DISPATCH(KERNEL, f, grid, s, a)                                                                                  \
    do {                                                                                                                     \
        const int sel = ((f).bps == 2 ? 4 : 0) | ((f).planar ? 2 : 0) | ((f).ch == 4 ? 1 : 0);                               \
        switch (sel) {                                                                                                       \
        case 0: hipLaunchKernelGGL((KERNEL<1, false, 3>), grid, dim3(256), 0, s, a); break;                                  \
        case 1: hipLaunchKernelGGL((KERNEL<1, false, 4>), grid, dim3(256), 0, s, a); break;                                  \
        case 2: hipLaunchKernelGGL((KERNEL<1, true, 3>), grid, dim3(256), 0, s, a); break;                                   \
        case 3: hipLaunchKernelGGL((KERNEL<1, true, 4>), grid, dim3(256), 0, s, a); break;                                   \
        case 4: hipLaunchKernelGGL((KERNEL<2, false, 3>), grid, dim3(256), 0, s, a); break;                                  \
        case 5: hipLaunchKernelGGL((KERNEL<2, false, 4>), grid, dim3(256), 0, s, a); break;                                  \
        case 6: hipLaunchKernelGGL((KERNEL<2, true, 3>), grid, dim3(256), 0, s, a); break;                                   \
        default: hipLaunchKernelGGL((KERNEL<2, true, 4>), grid, dim3(256), 0, s, a); break;                                  \
        }                                                                                                                    \
    } while (0)
