/*
 * srcnn_amd_yuv_packed_rect.h -- ONE RECTANGLE of a packed YUV frame's output (YUY2 / UYVY / YVYU, Y210 / Y212 / Y216, VUYA,
 * Y410, Y416, v210: what capture cards and SDI bridges deliver, and what a live viewer zooms and pans on or repaints a dirty
 * region of) at the cost of that rectangle, device-resident: the partial form of srcnn_yuv_packed_upscale_dev in both axes,
 * built on the window Y path of include/srcnn_amd_rect.h.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_yuv_packed.h and include/srcnn_amd_yuv_rect.h,
 * with a version of its own: the functions declared here are listed in include/srcnn_amd_yuv_packed_rect.abi, and
 * tests/test_yuv_packed_rect_abi.py holds header, list, binding and the library's export table to each other.  The older
 * headers are unchanged.
 *
 * Formats.  The ten SRCNN_YUVP_* formats of include/srcnn_amd_yuv_packed.h, which describes their layouts and values.
 *
 * Unit.  A packed row is made of units that cannot be half-written without reading the destination, and the library never
 * reads the destination: 2 pixels (a pixel pair) for YUY2 / UYVY / YVYU / Y210 / Y212 / Y216, 1 pixel for VUYA / Y410 / Y416,
 * 6 pixels (one 16-byte group) for v210.  A span of pixels [x, x + n) of a row of `width` pixels has x a multiple of the unit,
 * and n a multiple of the unit or x + n == width.
 *
 * Span.  srcnn_yuv_packed_span_bytes gives the unit, the byte offset of pixel x in its row and the byte length up to pixel
 * x + n.  When x + n == width the length runs to the end of the tight row (srcnn_yuv_packed_row_bytes): the empty second-Y
 * slot of an odd 4:2:2 width and v210's padding up to the end of the row's last 128-byte block are part of it.
 *
 * Result.  With (dw, dh) = srcnn_output_size(w, h, multiply, 0) and (off, n) = the span of pixels [x0, x0 + rw) of a dw-pixel
 * row, row r of the destination holds bytes [off, off + n) of row y0 + r of what srcnn_yuv_packed_upscale_dev writes for the
 * same frame, format, multiply and filter.  In SRCNN_MODE_STRICT that holds byte for byte, the zero bits beside the fields and
 * the zero slots at the right border included, whatever the rect -- the identity size, where chroma and alpha are copied,
 * included.  In the non-parity modes Y' is built from what srcnn_y_path_rect_f32_dev returns for the rect in that mode and
 * every other step is unchanged: the contract is exact in every mode.
 *
 * Alignment of the rect.  x0 and rw are under the unit rule against dw; y0 and rh are free.  Every other rect is SRCNN_E_ARG.
 *
 * Source.  src and src_pitch describe the WHOLE w x h frame, as for srcnn_yuv_packed_upscale_dev.
 *
 * Destination.  rh row segments of exactly n bytes; dst receives the byte at `off` of row y0 first.  A caller that repaints a
 * region inside a full-size packed dw x dh frame passes frame + y0 * pitch + off and the frame's pitch.  Pitches are in BYTES; 0
 * means tight (n bytes); a non-zero pitch is at least n.  dst and a non-zero pitch are multiples of the format's alignment (1,
 * 2 or 4: srcnn_yuv_packed_row_bytes).  Bytes outside the row segments are never written -- for a v210 rect that stops short of
 * dw, the groups between its last one and the end of the 128-byte block among them.
 *
 * Source rectangle.  srcnn_yuv_packed_rect_source reports, in LUMA pixel coordinates, [sx0, sx0 + sw) x [sy0, sy0 + sh): the
 * union of what the Y path reads for the rect (srcnn_y_path_rect_source: the rect, its halo of 6, the resampler's taps) and
 * what the taps of the chroma filter (box for SRCNN_FILTER_NEAREST, bilinear for every other filter; an axis that keeps its
 * size is copied) read for the chroma and alpha samples of the rect, expressed in luma columns, widened outward to the unit
 * and cut at w x h.  The call reads no byte of the source outside the span of pixels [sx0, sx0 + sw) of a w-pixel row
 * (srcnn_yuv_packed_span_bytes(format, w, sx0, sw, ...)) in rows [sy0, sy0 + sh): a caller may have only that part of the
 * frame valid.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call: it runs on the stream's context (srcnn_stream_create), or on the
 * calling thread's current context for NULL or a raw HIP stream.
 *
 * Scratch comes from that stream's grow-only workspace, stays there until srcnn_trim, and scales with the window, never with
 * w * h or dw * dh.  With band = rh, or the rows of one pass when the rect is banded (below), ysrc = the samples of the Y
 * path's source rectangle, usrc = sw * sh of the source rectangle above and p = 2 planes' worth for the 4:2:2 formats (Y, and U
 * + V of half the width each), 4 for 4:4:4 + alpha, the call retains, beside what srcnn_y_path_rect_f32_dev retains for the
 * rect (include/srcnn_amd_rect.h),
 *     4 * (ysrc + rw * band)                bytes when the chroma grid is up-scaled in both axes (chroma and alpha are resampled
 *                                           tile by tile from the packed source; no float chroma or alpha plane exists), and
 *     4 * p * (usrc + rw * band)            bytes for every other shape (down-scales, mixed axes, the identity size, tables of
 *                                           more than 8 taps) and with SRCNN_YUV_PACKED_RECT_UNFUSED=1, which sends every
 *                                           shape that way
 * (each float plane's start rounded up to 256 bytes).  Both routes give the same bytes.  All ten formats take the first route
 * by default where the shape allows it (profiles/yuv_packed_rect_probe.txt).
 *
 * Bands.  When the 32 layer-2 planes of the window exceed the workspace cap (srcnn_set_workspace_limit), the rect is produced
 * in the horizontal bands of srcnn_y_path_rect_f32_dev, with identical bytes; a packed row mixes luma and chroma, so chroma
 * and alpha are merged band by band.
 *
 * Errors (all before any device lookup, in this order):
 *   SRCNN_E_ARG          unknown format; NULL src or dst, zero rw / rh, unknown filter, zero w / h
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^23 - 1 output columns, 2^31 - 1 pixels)
 *   SRCNN_E_ARG          a rect that is not inside dw x dh (x0 + rw and y0 + rh are taken without 32-bit wrap); then a rect
 *                        that breaks the unit rule; then a pitch below its row (the tight row of the source, n of the
 *                        destination), a base address or pitch that is not a multiple of the format's alignment; then source
 *                        and destination byte ranges that overlap (the range of a side is pitch * (rows - 1) + its row bytes)
 *   SRCNN_E_NODEVICE     no gfx950 device
 * srcnn_yuv_packed_rect_source returns the geometry errors among these (format, filter, sizes, scale, limits, rect, unit
 * rule); srcnn_yuv_packed_span_bytes returns SRCNN_E_ARG for an unknown format, a zero width or n, pixels outside the row and
 * a span that breaks the unit rule.  A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_YUV_PACKED_RECT_H
#define SRCNN_AMD_YUV_PACKED_RECT_H

#include <stddef.h>

#include "srcnn_amd_yuv_packed.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_YUV_PACKED_RECT_VERSION 1

int srcnn_yuv_packed_rect_abi_version(void);   /* SRCNN_AMD_YUV_PACKED_RECT_VERSION of the loaded library */
/* pure, no device: for a row of `width` pixels in `format`, the unit (in pixels) that spans are made of, and the byte offset
 * and byte length of pixels [x, x + n).  Any result pointer may be NULL. */
int srcnn_yuv_packed_span_bytes(int format, unsigned width, unsigned x, unsigned n,
                                unsigned* unit, size_t* byte_offset, size_t* bytes);
/* pure, no device: the source rectangle, in LUMA pixel coordinates, that the output rect depends on.  Any result pointer may
 * be NULL. */
int srcnn_yuv_packed_rect_source(int format, unsigned w, unsigned h, float multiply, int filter,
                                 unsigned x0, unsigned y0, unsigned rw, unsigned rh,
                                 unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh);
int srcnn_yuv_packed_upscale_rect_dev(int format, unsigned w, unsigned h, float multiply, int filter,
                                      const void* src, size_t src_pitch,                    /* the WHOLE w x h frame */
                                      unsigned x0, unsigned y0, unsigned rw, unsigned rh,   /* in luma output coordinates */
                                      void* dst, size_t dst_pitch, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_YUV_PACKED_RECT_H */
