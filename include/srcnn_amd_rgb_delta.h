/*
 * srcnn_amd_rgb_delta.h -- UPSCALE ONLY WHAT CHANGED between two RGB(A) images that are both in device memory: the library finds
 * on the device which tiles of the output can differ, and repaints those through the RGB(A) rect list call
 * (include/srcnn_amd_rgb_rect_list.h) inside the caller's full-size output image.  The RGB(A) counterpart of
 * include/srcnn_amd_delta.h, for callers that hold last frame and this frame as integer pixel surfaces but no list of dirty
 * rectangles: remote desktops, screen capture, UI compositors.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_delta.h and include/srcnn_amd_rgb_rect_list.h,
 * with a version of its own: the functions declared here are listed in include/srcnn_amd_rgb_delta.abi, and
 * tests/test_rgb_delta_abi.py holds header, list, binding and the library's export table to each other.  The older headers are
 * unchanged.
 *
 * The contract.  With (dw, dh) = srcnn_output_size(w, h, multiply, 0), a grid of tile_w x tile_h output pixels covers dw x dh:
 * cols = ceil(dw / tile_w), rows = ceil(dh / tile_h), the last column and row may be partial.  tile_w / tile_h: 0 = 64, otherwise
 * 8 ... 65535.  Tile (c, r) is DIRTY if and only if some pixel inside srcnn_rgb_rect_source(w, h, multiply, filter, <tile c,r>)
 * has a byte that differs between prev and cur, in any byte of any of its samples.  Alpha counts.  At depth > 8 both bytes of a
 * 16-bit word count, unused high bits included: the rule is about bytes, not values.  The definition is exact, not merely
 * conservative: a pixel outside a tile's source rectangle never flags it, whatever word or vector it shares with one inside.
 * Bytes between a row and its pitch are never read.
 *
 * Result of srcnn_rgb_upscale_delta_dev.  In SRCNN_MODE_STRICT: if dst (and dst_conv) held srcnn_rgb_upscale_dev of the previous
 * image, they now hold it for the current one, byte for byte -- the rect call's result depends on no source sample outside the
 * rectangle srcnn_rgb_rect_source reports, and a rect is a crop of the whole image, so this is not an approximation.  Pixels of
 * clean tiles are not written at all, and neither are bytes between a row's dw pixels and its pitch.  In the other modes a pixel
 * is either untouched or what srcnn_rgb_upscale_rect_dev gives in that mode.
 *
 * How.  One kernel reads every byte of both images once and sets a byte per dirty tile; the flags are copied to the host; maximal
 * runs of dirty tiles of a tile row that repeat in the next row are joined into rects (srcnn_rgb_delta_rects is that rule, the
 * one of srcnn_y_path_delta_rects); srcnn_rgb_upscale_rect_list_dev repaints them.  The image is repainted as the single rect
 * (0, 0, dw, dh) instead when every tile is dirty, when there are more than 65536 rects, or when the sum of (rw + 12) * (rh + 12)
 * over the rects reaches SRCNN_DELTA_WHOLE_PERMILLE / 1000 of dw * dh (the setting of include/srcnn_amd_delta.h).  Either route
 * gives the same bytes.
 *
 * Stream.  srcnn_rgb_delta_flags_dev is asynchronous on `stream`, like every *_dev call (its first call with a new geometry
 * uploads the span tables with a blocking copy, as a first call with a new size uploads its resampling tables).
 * srcnn_rgb_upscale_delta_dev BLOCKS THE HOST until the flags have arrived -- one synchronisation of `stream`, so everything
 * queued on it before has finished too -- and queues the upscale itself asynchronously.  On a stream that the caller is capturing
 * into a graph it returns SRCNN_E_UNSUPPORTED before anything is queued: a capture cannot wait.  srcnn_rgb_delta_flags_dev can be
 * captured once it has run with the same geometry on that stream outside a capture; otherwise SRCNN_E_UNSUPPORTED.
 *
 * Memory.  Format, planes and samples are those of include/srcnn_amd_rgb.h.  prev, cur: whole w x h images in fmt (prev == NULL,
 * the array pointer: no previous image); dst (and dst_conv): the whole dw x dh image; d_flags: cols * rows bytes, row-major, each
 * 0 or 1 after the call, no byte outside written.  Pitches are in BYTES; 0 (or a NULL pitch array) means tight rows; a non-zero
 * pitch is at least the row.  At depth 8 bases need no alignment; above 8 every base address and every non-zero pitch is even.
 * Where every base and every pitch of both images is a multiple of 16 (one row: every base) the kernel reads 16 bytes per lane
 * and image at a time.
 * Scratch comes from the stream's grow-only workspace and stays there until srcnn_trim: 8 * (cols + rows) bytes of tables,
 * cols * rows flag bytes on the device and page-locked on the host, and what include/srcnn_amd_rgb_rect_list.h states for the
 * rects.
 *
 * Errors, all before any device lookup, in this order:
 *   SRCNN_E_ARG          NULL fmt, struct_size other than sizeof(srcnn_rgb_format), unknown layout / order / alpha / depth
 *   SRCNN_E_ARG          unknown filter, zero w / h
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^23 - 1 output columns, 2^31 - 1 pixels)
 *   SRCNN_E_ARG          a tile side of 1 ... 7 or above 65535
 *   SRCNN_E_UNSUPPORTED  more than 2048 tile columns or tile rows (the kernel holds both span tables in LDS)
 *   SRCNN_E_ARG          stats->struct_size != sizeof(srcnn_delta_stats)
 *   SRCNN_E_ARG          NULL cur or d_flags, a NULL required plane of prev or cur; a source pitch below its row, at depth > 8
 *                        an odd source base address or pitch
 *   SRCNN_E_ARG          NULL dst or required destination plane; a destination pitch below its row of dw pixels, at depth > 8
 *                        an odd base address or pitch; then any source plane of either image whose byte range overlaps that of
 *                        a destination plane (dst_conv counts as one); then two destination planes that overlap each other
 *   SRCNN_E_UNSUPPORTED  a stream under the caller's capture (see Stream)
 *   SRCNN_E_NODEVICE     no gfx950 device (the device calls only)
 * srcnn_rgb_delta_rects: SRCNN_E_ARG for NULL n, NULL flags, a grid that does not cover dw x dh, a tile side outside 8 ... 65535,
 * items == NULL with cap > 0, item_size != sizeof(srcnn_rgb_rect_item), a pitch below its row or (depth > 8) an odd base or
 * pitch, cap below the number of rects (*n is set); SRCNN_E_SCALE for a zero dw or dh.
 * A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_RGB_DELTA_H
#define SRCNN_AMD_RGB_DELTA_H

#include <stddef.h>

#include "srcnn_amd_delta.h"
#include "srcnn_amd_rgb_rect_list.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_RGB_DELTA_VERSION 1

int srcnn_rgb_delta_abi_version(void);   /* SRCNN_AMD_RGB_DELTA_VERSION of the loaded library */
/* pure, no device: checks the geometry and reports the output size and the tile grid with the defaults applied.  Any of the four
 * results may be NULL. */
int srcnn_rgb_delta_grid(unsigned w, unsigned h, float multiply, int filter, unsigned tile_w, unsigned tile_h,
                         unsigned* dw, unsigned* dh, unsigned* cols, unsigned* rows);
/* the dirty flags of the grid, cols * rows bytes at d_flags.  prev == NULL: "no previous image" -- all ones, cur is not read */
int srcnn_rgb_delta_flags_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                              const void* const prev[4], const size_t prev_pitch[4],
                              const void* const cur[4], const size_t cur_pitch[4],
                              unsigned tile_w, unsigned tile_h, unsigned char* d_flags, void* stream);
/* pure host, the coalescer: HOST flags (non-zero = dirty) of a cols x rows grid of tile_w x tile_h tiles (both given, not 0) over
 * dw x dh into rects whose items point into the full-size image dst / dst_conv in fmt: an item's dst[p] (and dst_conv) is the
 * address of pixel (x0, y0) of the image, with the image's pitch (0 = tight rows of dw pixels).  dst == NULL: NULL destinations.
 * The rects are pairwise disjoint, their union is exactly the dirty tiles clipped to dw x dh.  *n: their number; items == NULL
 * with cap == 0 counts only.  item_size: sizeof(srcnn_rgb_rect_item).  It does not apply the whole-frame rule. */
int srcnn_rgb_delta_rects(const unsigned char* flags, unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h,
                          const srcnn_rgb_format* fmt, unsigned dw, unsigned dh,
                          void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch,
                          srcnn_rgb_rect_item* items, unsigned cap, unsigned item_size, unsigned* n);
/* the whole operation.  prev == NULL: the whole image.  stats may be NULL */
int srcnn_rgb_upscale_delta_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                const void* const prev[4], const size_t prev_pitch[4],
                                const void* const cur[4], const size_t cur_pitch[4],
                                unsigned tile_w, unsigned tile_h,
                                void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch,
                                void* stream, srcnn_delta_stats* stats);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_RGB_DELTA_H */
