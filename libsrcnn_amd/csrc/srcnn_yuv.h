// srcnn_yuv.h -- internal interface of the YUV conversion kernels: planar and semi-planar frames of every supported depth
// (srcnn_yuv_planes.hip), their chroma over a window (srcnn_yuv_window.hip), packed frames (srcnn_yuv_packed.hip) and packed frames
// over a window (srcnn_yuv_packed_window.hip).  The rules the launchers take are srcnn_frame_rules.h; the host
// side is srcnn_frames.cpp.  Not installed; the public surface is include/srcnn_amd_yuv.h, srcnn_amd_yuv_ex.h and
// srcnn_amd_yuv_packed.h; the rect calls are include/srcnn_amd_yuv_rect.h and include/srcnn_amd_yuv_packed_rect.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "srcnn_frame_rules.h"
#include "srcnn_kernels.h"

namespace srcnn {

// ---- planes (srcnn_yuv_planes.hip).  f == NULL: 8-bit samples; else 16-bit words read and written by *f (base and pitch even) ----
// Pitched plane -> tight float plane(s), rows [0, rows).  uv = false: `w` samples per row -> d0.  uv = true: `w` interleaved
// (U, V) pairs per row -> d0 (U) and d1 (V).  luma (16-bit only): the values are multiplied by f->down; chroma stays on the
// native scale.
void launch_plane_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, bool uv, const Yuv16Rule* f, bool luma,
                         float* d0, float* d1, hipStream_t s);
// Tight float rows -> pitched plane, rows [0, rows) of the source to destination rows [row0, row0 + rows).
// sat = false: (unsigned char) v or (unsigned)(v * f->up) (Y': layer 3 already clamps); sat = true: MIN(maxv), MAX(0),
// truncation (chroma).  s1 != NULL: `w` pairs (s0[i], s1[i]) interleaved per row, saturated.
void launch_plane_pack(const float* s0, const float* s1, unsigned w, unsigned rows, bool sat, const Yuv16Rule* f,
                       unsigned char* dst, size_t pitch, unsigned row0, hipStream_t s);

// ---- the window form behind the rect call (srcnn_yuv_window.hip; include/srcnn_amd_yuv_rect.h) ----
// U' and V' of chroma output columns [cx0, cx0 + cols) and rows [cy0, cy0 + rows) resampled from the WHOLE cw x ch integer
// chroma plane(s) src with the tables th (columns) and tv (rows), an up-scale in both axes, saturated and written as
// launch_plane_pack writes chroma, into dst, whose first sample is the rect's.  semi: src[0] / dst[0] hold (U, V) pairs, else
// src[0] / dst[0] are U and src[1] / dst[1] V.  f as for launch_plane_unpack.  No source byte outside the taps' span is read.
// The caller has asked window_tile_fits (srcnn_window_tile.h) for that range.
void launch_yuv_window_chroma(const unsigned char* const src[2], const size_t spitch[2], unsigned cw, unsigned ch, bool semi,
                              const Yuv16Rule* f, unsigned cx0, unsigned cy0, unsigned cols, unsigned rows, const DevAxisTable& th,
                              const DevAxisTable& tv, unsigned char* const dst[2], const size_t dpitch[2], hipStream_t s);

// ---- the three kernels of the rect LIST call (srcnn_yuv_rect_list.hip; include/srcnn_amd_yuv_rect_list.h) ----
struct ListCellDesc;         // srcnn_rect_atlas.hpp
struct YuvListDstDesc;       // srcnn_yuv_rect_atlas.hpp
// launch_list_resample (srcnn_rect_list.h) reading Y off the pitched integer luma plane src (the WHOLE w x h plane) as
// launch_plane_unpack reads luma.  th, tv: the Y tables.  f as for launch_plane_unpack.
void launch_yuv_list_resample(const unsigned char* src, size_t spitch, unsigned w, unsigned h, const Yuv16Rule* f, const DevAxisTable& th,
                              const DevAxisTable& tv, const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas,
                              unsigned atlas_w, hipStream_t s);
// Every rect of a pass: Y' of the atlas result written as launch_plane_pack writes luma (sat = false) where dd (the device copy
// of the pass's destination table, entry k for cell k) points.
void launch_yuv_list_luma(const Yuv16Rule* f, const ListCellDesc* d, const YuvListDstDesc* dd, unsigned ncells, const ListCellDesc& end,
                          const float* atlas, unsigned atlas_w, hipStream_t s);
// Every chroma rect of a pass: launch_yuv_window_chroma for the chroma rect and the planes of each entry of dd; `end`: the
// table's closing entry (the tile total).  The router has asked window_tile_fits for every chroma rect.
void launch_yuv_list_chroma(const unsigned char* const src[2], const size_t spitch[2], unsigned cw, unsigned ch, bool semi, const Yuv16Rule* f,
                            const DevAxisTable& cth, const DevAxisTable& ctv, const YuvListDstDesc* dd, unsigned ncells,
                            const YuvListDstDesc& end, hipStream_t s);

// ---- packed frames: one plane that interleaves Y, U, V (and A) (srcnn_yuv_packed.hip) ----
// Packed rows [0, rows) of `w` pixels -> tight float planes: dy (w per row, scaled by f.down), du / dv (ceil(w/2) per row for
// the 4:2:2 kinds, else w; native scale), da (w per row; only where f.amask).  Base and pitch must have the format's alignment.
void launch_yuvp_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, const YuvPackedRule& f, float* dy,
                        float* du, float* dv, float* da, hipStream_t s);
// Tight float rows [0, rows) of sy, su, sv (sa) -> packed destination rows [row0, row0 + rows); every byte of those tight rows
// is written once, slots without a sample as zero.  Y': (unsigned)(v * f.up); chroma and alpha: MIN(maxv), MAX(0), truncation.
// span_bytes != 0 (the rect call): only the first span_bytes bytes of each row are written -- yuv_packed_span of the rect, which
// for v210 stops at the rect's last group instead of the 128-byte block's end unless the rect reaches the right border.
void launch_yuvp_pack(const float* sy, const float* su, const float* sv, const float* sa, unsigned w, unsigned rows,
                      const YuvPackedRule& f, unsigned char* dst, size_t pitch, unsigned row0, hipStream_t s, size_t span_bytes = 0);

// ---- the window form behind the packed rect call (srcnn_yuv_packed_window.hip; include/srcnn_amd_yuv_packed_rect.h) ----
// Luma columns [sx0, sx0 + sw) of rows [sy0, sy0 + sh) of the WHOLE w-pixel-wide packed frame src -> the tight float window y (sw
// floats per row), (float)field * f.down: the Y half of launch_yuvp_unpack.  No byte outside yuv_packed_span of those columns
// widened to the format's unit is read.
void launch_yuvp_window_y(const YuvPackedRule& f, const unsigned char* src, size_t pitch, unsigned w, unsigned sx0, unsigned sy0, unsigned sw,
                          unsigned sh, float* y, hipStream_t s);
// One band of a rect: U', V' (and A') of chroma output columns [cx0, cx0 + ccols) and output rows [gy0, gy0 + rows) resampled from
// the WHOLE packed w x h frame with the tables th (chroma columns) and tv (rows), an up-scale in both axes of the chroma grid,
// merged with the band's finished Y' rows (yband: tight, rw floats per row; luma column yuv_packed_chroma_step * cx0 first) and
// written as launch_yuvp_pack writes them into rows [row0, row0 + rows) of dst, whose first byte is the rect's first;
// span_bytes: bytes of a row segment (yuv_packed_span of the rect).  The caller has asked yuvp_window_fits for every band.
void launch_yuvp_window_merge(const YuvPackedRule& f, const unsigned char* src, size_t spitch, unsigned w, unsigned h, const float* yband,
                              unsigned cx0, unsigned gy0, unsigned rw, unsigned ccols, unsigned rows, const DevAxisTable& th,
                              const DevAxisTable& tv, unsigned char* dst, size_t dpitch, unsigned row0, size_t span_bytes, hipStream_t s);

// ---- the two kernels of the packed rect LIST call (srcnn_yuv_packed_rect_list.hip; include/srcnn_amd_yuv_packed_rect_list.h) ----
struct YuvPackedListDstDesc; // srcnn_yuv_packed_rect_atlas.hpp
// launch_list_resample (srcnn_rect_list.h) reading Y off the WHOLE packed w x h frame src as launch_yuvp_window_y reads it, one
// dword per sample.  th, tv: the Y tables.
void launch_yuvp_list_resample(const YuvPackedRule& f, const unsigned char* src, size_t spitch, unsigned w, unsigned h, const DevAxisTable& th,
                               const DevAxisTable& tv, const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas,
                               unsigned atlas_w, hipStream_t s);
// Every rect of a pass: launch_yuvp_window_merge for all rows of the rect of each entry of dd (the device copy of the pass's
// destination table, entry k for cell k of d), Y' read from the cell of the layer-3 atlas; `end`: the table's closing entry (the
// tile total).  cth, ctv: the chroma tables (dcw <- cw), (dh <- h).  The router has asked yuvp_window_fits for every item.
void launch_yuvp_list_merge(const YuvPackedRule& f, const unsigned char* src, size_t spitch, unsigned w, unsigned h, const DevAxisTable& cth,
                            const DevAxisTable& ctv, const ListCellDesc* d, const YuvPackedListDstDesc* dd, unsigned ncells,
                            const YuvPackedListDstDesc& end, const float* atlas, unsigned atlas_w, hipStream_t s);

}  // namespace srcnn
