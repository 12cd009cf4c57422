/*
 * srcnn_amd_yuv_rect.h -- ONE RECTANGLE of a planar or semi-planar YUV frame's output (the viewport of a player that zooms or
 * pans, a dirty region of a compositor, a tile of an 8K transcode) at the cost of that rectangle, device-resident: the partial
 * form of srcnn_yuv_upscale_dev in both axes, built on the window Y path of include/srcnn_amd_rect.h.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_yuv_ex.h and include/srcnn_amd_rect.h, with a
 * version of its own: the functions declared here are listed in include/srcnn_amd_yuv_rect.abi, and
 * tests/test_yuv_rect_abi.py holds header, list, binding and the library's export table to each other.  The older headers
 * are unchanged.
 *
 * Formats.  Every srcnn_yuv_format srcnn_yuv_upscale_dev takes: planar or semi-planar, 4:2:0 / 4:2:2 / 4:4:4, depth 8 / 10 /
 * 12 / 14 / 16, the value in the low or the high end of a 16-bit word (8-bit 4:2:0 is I420 and NV12).
 *
 * Result.  With (dw, dh) = srcnn_output_size(w, h, multiply, 0), the luma rect is [x0, x0 + rw) x [y0, y0 + rh) of the dw x dh
 * output, and the chroma rect is the set of chroma samples that cover it: columns [x0 / 2, (x0 + rw + 1) / 2) where the format
 * subsamples horizontally (4:2:0, 4:2:2), rows [y0 / 2, (y0 + rh + 1) / 2) for 4:2:0, the luma rect itself on an axis that is
 * not subsampled.  Every sample written is the sample srcnn_yuv_upscale_dev writes at that position for the same frame,
 * format, multiply and filter.  In SRCNN_MODE_STRICT that holds byte for byte, the zero bits beside the value included,
 * whatever the rect -- the identity size, where chroma is copied, included.  In the non-parity modes Y' is built from what
 * srcnn_y_path_rect_f32_dev returns for that rect in that mode and every other step is unchanged: the contract is exact in
 * every mode.
 *
 * Alignment of the rect.  x0 is even where chroma is subsampled horizontally, y0 is even for 4:2:0; rw and rh are free.  An odd
 * width that does not reach the right border writes one chroma column whose second luma column lies outside the rect: that
 * chroma sample is still the whole frame's value.  The same holds for rows.  So the destination planes are exactly those of
 * an rw x rh frame in fmt: srcnn_yuv_plane_size(fmt, rw, rh, plane, ...) gives their columns, rows and tight row bytes.
 *
 * Source.  src and src_pitch describe the WHOLE w x h frame, as for srcnn_yuv_upscale_dev.
 *
 * Destination.  dst[0] receives luma sample (x0, y0) first; dst[1] and dst[2] receive chroma sample (x0 / 2, y0 / 2) first
 * (each axis under its own subsampling), a UV plane that U, V pair.  A caller that repaints a region inside a full-size
 * dw x dh frame passes the addresses of those samples as the plane bases and the frame's pitches.  Pitches are in BYTES; 0 (or
 * a NULL pitch array) means tight rows of the rect; a non-zero pitch is at least the row of rw luma samples (of the chroma
 * rect's columns).  At depth 8 bases need no alignment; above 8 every base address and every non-zero pitch is even.  Bytes
 * outside those row segments are never written.
 *
 * Source rectangle.  srcnn_yuv_rect_source reports, per plane and in that plane's own sample coordinates (a UV plane: one
 * column per U, V pair), what the rect depends on.  Plane 0: what srcnn_y_path_rect_source(w, h, dw, dh, filter, ...) reports
 * (the rect, its halo of 6, the resampler's taps).  Chroma planes: the first to last tap the chroma filter's contribution
 * tables (ceil(dw/2) <- ceil(w/2) columns, likewise rows, under the format's subsampling) give for the chroma rect -- box for
 * SRCNN_FILTER_NEAREST, bilinear for every other filter; an axis that keeps its size is copied.  Plane 2 of a semi-planar
 * frame: 0 x 0.  The call reads no byte of any source plane outside that plane's rectangle: a caller may have only that part
 * of the frame valid.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call: it runs on the stream's context (srcnn_stream_create), or on the
 * calling thread's current context for NULL or a raw HIP stream.
 *
 * Scratch comes from that stream's grow-only workspace, stays there until srcnn_trim, and scales with the window, never with
 * w * h or dw * dh.  With band = rh, or the rows of one pass when the rect is banded (below), ysrc = the samples of plane 0's
 * source rectangle, csrc = the samples of one chroma plane's source rectangle and crect = the samples of the chroma rect, the
 * call retains, beside what srcnn_y_path_rect_f32_dev retains for the rect (include/srcnn_amd_rect.h),
 *     4 * (ysrc + rw * band)                        bytes when chroma is up-scaled in both axes (it is resampled tile by tile
 *                                                   from the integer source; no float chroma plane exists), and
 *     4 * (ysrc + rw * band + 2 * (csrc + crect))   bytes for every other shape (down-scales, mixed axes, the identity size)
 *                                                   and with SRCNN_YUV_RECT_UNFUSED=1, which sends every shape that way
 * (each float plane's start rounded up to 256 bytes).  Both routes give the same bytes.  For a 960 x 512 rect of a
 * 3840 x 2160 -> 7680 x 4320 4:2:0 frame the first line is 2.5 MB and the second adds 1.2 MB; srcnn_yuv_upscale_dev retains
 * 4.6 GB for that frame.
 *
 * Bands.  When the 32 layer-2 planes of the window exceed the workspace cap (srcnn_set_workspace_limit), the luma rect is
 * produced in the horizontal bands of srcnn_y_path_rect_f32_dev, with identical bytes; chroma does not follow the bands.
 *
 * Errors (all before any device lookup, in this order):
 *   SRCNN_E_ARG          NULL fmt, struct_size other than sizeof(srcnn_yuv_format), unknown layout / chroma / depth,
 *                        msb_aligned other than 0 / 1 or set at depth 8; NULL plane array or required plane, zero rw / rh,
 *                        unknown filter, zero w / h
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^23 - 1 output columns, 2^31 - 1 pixels)
 *   SRCNN_E_ARG          a rect that is not inside dw x dh (x0 + rw and y0 + rh are taken without 32-bit wrap); then an odd x0
 *                        (4:2:0, 4:2:2) or odd y0 (4:2:0); then a pitch below its row, at depth > 8 an odd base address or odd
 *                        pitch; then any source plane whose whole byte range overlaps that of a destination plane (the range
 *                        of a plane is pitch * (rows - 1) + its row bytes), or two destination planes that overlap each other
 *   SRCNN_E_NODEVICE     no gfx950 device
 * srcnn_yuv_rect_source returns the geometry errors among these (format, filter, sizes, scale, limits, rect, odd origin), and
 * SRCNN_E_ARG for a plane outside 0..2.  A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_YUV_RECT_H
#define SRCNN_AMD_YUV_RECT_H

#include <stddef.h>

#include "srcnn_amd_yuv_ex.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_YUV_RECT_VERSION 1

int srcnn_yuv_rect_abi_version(void);   /* SRCNN_AMD_YUV_RECT_VERSION of the loaded library */
/* pure, no device: for `plane` (0..2), in that plane's own sample coordinates (a UV plane: one column per U,V pair), the source
 * rectangle [*sx0, *sx0 + *sw) x [*sy0, *sy0 + *sh) the output rect depends on.  Plane 2 of a semi-planar frame: 0 x 0.  Any
 * result pointer may be NULL. */
int srcnn_yuv_rect_source(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                          unsigned x0, unsigned y0, unsigned rw, unsigned rh, int plane,
                          unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh);
int srcnn_yuv_upscale_rect_dev(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                               const void* const src[3], const size_t src_pitch[3],   /* the WHOLE w x h frame */
                               unsigned x0, unsigned y0, unsigned rw, unsigned rh,     /* in luma output coordinates */
                               void* const dst[3], const size_t dst_pitch[3],         /* an rw x rh frame in fmt */
                               void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_YUV_RECT_H */
