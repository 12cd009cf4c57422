/*
 * srcnn_amd_rgb_rect.h -- ONE RECTANGLE of an RGB(A) image's output (a viewport, a dirty rectangle of a UI surface, a tile of
 * an image larger than the scratch budget) at the cost of that rectangle, device-resident: the partial form of
 * srcnn_rgb_upscale_dev in both axes, built on the window Y path of include/srcnn_amd_rect.h.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_rgb.h and include/srcnn_amd_rect.h, with a
 * version of its own: the functions declared here are listed in include/srcnn_amd_rgb_rect.abi, and
 * tests/test_rgb_rect_abi.py holds header, list, binding and the library's export table to each other.  The older headers
 * are unchanged.
 *
 * Result.  With (dw, dh) = srcnn_output_size(w, h, multiply, 0), pixel (i, j) of dst and of dst_conv, i < rw, j < rh, is
 * pixel (x0 + i, y0 + j) of what srcnn_rgb_upscale_dev writes for the same image, format, multiply and filter.  In
 * SRCNN_MODE_STRICT that holds byte for byte, whatever the rect -- the identity size, where chroma is copied (the library's
 * pinned identity-size deviation), included.  Format, planes, samples and every value formula are those of
 * include/srcnn_amd_rgb.h.  In the non-parity modes Y' is what srcnn_y_path_rect_f32_dev returns for that rect in that mode
 * and every other step is unchanged: the contract is exact in every mode.
 *
 * Source.  src and src_pitch describe the WHOLE w x h image, as for srcnn_rgb_upscale_dev.
 *
 * Destination.  dst (and dst_conv) is an rw x rh image in fmt: pixel (x0, y0) of the output comes first.  A caller that
 * repaints a dirty rectangle inside a full-size dw x dh image passes the address of that image's pixel (x0, y0) as the plane
 * base and the image's pitch.  Pitches are in BYTES; 0 (or a NULL pitch array) means tight rows of rw pixels; a non-zero
 * pitch is at least the row of rw pixels.  At depth 8 bases need no alignment; above 8 every base address and every non-zero
 * pitch is even.  Bytes outside the rw pixels of a row are never written.
 *
 * Source rectangle.  srcnn_rgb_rect_source reports the union of what srcnn_y_path_rect_source(w, h, dw, dh, filter, ...)
 * reports for the Y path (the rect, its halo of 6, the resampler's taps) and of the first and last tap the chroma filter's
 * contribution tables give for columns [x0, x0 + rw) and rows [y0, y0 + rh) (box for SRCNN_FILTER_NEAREST, bilinear for
 * every other filter; an axis that keeps its size is copied).  The result depends on no source sample outside that
 * rectangle, and the call reads no byte of any source plane outside it: a caller may have only that part of the image valid.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call: it runs on the stream's context (srcnn_stream_create), or on the
 * calling thread's current context for NULL or a raw HIP stream.
 *
 * Scratch comes from that stream's grow-only workspace, stays there until srcnn_trim, and scales with the window, never with
 * w * h or dw * dh.  With band = rh, or the rows of one pass when the rect is banded (below), ysrc = the samples of the Y
 * path's source rectangle, usrc = the samples of the rectangle srcnn_rgb_rect_source reports and c = 3 + alpha, the call
 * retains, beside what srcnn_y_path_rect_f32_dev retains for the rect (include/srcnn_amd_rect.h),
 *     4 * (ysrc + rw * band)            bytes for an up-scale in both axes (chroma and alpha are resampled tile by tile from
 *                                       the integer source; no float plane of them exists), and
 *     4 * c * (usrc + rw * band)        bytes for every other shape (down-scales, mixed axes, the identity size) and with
 *                                       SRCNN_RGB_RECT_UNFUSED=1, which sends every shape that way.
 * Both routes give the same bytes.
 *
 * Bands.  When the 32 layer-2 planes of the window exceed the workspace cap (srcnn_set_workspace_limit), the rect is produced
 * in the horizontal bands of srcnn_y_path_rect_f32_dev, colour included, with identical bytes.
 *
 * Errors (all before any device lookup, in this order):
 *   SRCNN_E_ARG          NULL fmt, struct_size other than sizeof(srcnn_rgb_format), unknown layout / order / alpha / depth,
 *                        NULL plane array or required plane, zero rw / rh, unknown filter, zero w / h
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^23 - 1 output columns, 2^31 - 1 pixels)
 *   SRCNN_E_ARG          a rect that is not inside dw x dh (x0 + rw and y0 + rh are taken without 32-bit wrap);
 *                        then a pitch below its row (destination rows are rw pixels), at depth > 8 an odd base address or odd
 *                        pitch; then any source plane whose whole byte range overlaps that of a destination plane (dst_conv
 *                        counts as one; the range of a destination plane is pitch * (rh - 1) + its row bytes), or two
 *                        destination planes that overlap each other
 *   SRCNN_E_NODEVICE     no gfx950 device
 * srcnn_rgb_rect_source returns the geometry errors among these (filter, sizes, scale, limits, rect).
 * A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_RGB_RECT_H
#define SRCNN_AMD_RGB_RECT_H

#include <stddef.h>

#include "srcnn_amd_rgb.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_RGB_RECT_VERSION 1

int srcnn_rgb_rect_abi_version(void);   /* SRCNN_AMD_RGB_RECT_VERSION of the loaded library */
/* pure, no device: the source rectangle [*sx0, *sx0 + *sw) x [*sy0, *sy0 + *sh) the output rect depends on.  Any of the four
 * results may be NULL. */
int srcnn_rgb_rect_source(unsigned w, unsigned h, float multiply, int filter,
                          unsigned x0, unsigned y0, unsigned rw, unsigned rh,
                          unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh);
int srcnn_rgb_upscale_rect_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                               const void* const src[4], const size_t src_pitch[4],   /* the WHOLE w x h source image */
                               unsigned x0, unsigned y0, unsigned rw, unsigned rh,     /* in output (dw x dh) coordinates */
                               void* const dst[4], const size_t dst_pitch[4],         /* an rw x rh image: pixel (x0, y0) first */
                               void* dst_conv, size_t dst_conv_pitch,                 /* optional rw x rh truncated Y', NULL: none */
                               void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_RGB_RECT_H */
