/*
 * srcnn_amd_yuv_packed_rect_list.h -- A LIST OF RECTANGLES of a packed YUV frame's output in one call (the dirty rectangles of
 * a capture surface in a live viewer or a compositor: YUY2 / UYVY / YVYU, Y210 / Y212 / Y216, VUYA, Y410, Y416, v210),
 * device-resident: srcnn_yuv_packed_upscale_rect_dev (include/srcnn_amd_yuv_packed_rect.h) for many rects at the launch cost of
 * a few, built on the atlas of include/srcnn_amd_rect_list.h.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_yuv_packed_rect.h, include/srcnn_amd_rect_list.h,
 * include/srcnn_amd_rgb_rect_list.h and include/srcnn_amd_yuv_rect_list.h, with a version of its own: the functions declared
 * here are listed in include/srcnn_amd_yuv_packed_rect_list.abi, and tests/test_yuv_packed_rect_list_abi.py holds header, list,
 * binding and the library's export table to each other.  The older headers are unchanged.  With this header every surface kind
 * (Y plane, RGB(A), planar / semi-planar YUV, packed YUV) has a rect call and a rect list call.
 *
 * Result.  After the call item k holds exactly what
 *     srcnn_yuv_packed_upscale_rect_dev(format, w, h, multiply, filter, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, stream)
 * would have written for that item's rect and dst, at the current numerics mode (srcnn_set_mode): in SRCNN_MODE_STRICT byte
 * for byte, the zero bits beside the fields, the empty second-Y slot of an odd 4:2:2 width and v210's padding groups where a
 * rect reaches the right border included -- i.e. every item is a crop, by srcnn_yuv_packed_span_bytes, of what
 * srcnn_yuv_packed_upscale_dev writes for the whole frame -- and in the other modes by construction, because there the list runs
 * that call item by item.  Bytes outside an item's row segments are never written, the groups between a v210 rect that stops
 * short of dw and the end of its 128-byte block among them.  The destination is never read.  Formats, the unit rule, the span
 * and every value formula are those of include/srcnn_amd_yuv_packed_rect.h.
 *
 * How.  A BATCHED item shares the layer kernels' launches with the others through the atlas of include/srcnn_amd_rect_list.h:
 * the same cells of (rw + 12) x (rh + 12) samples, the same packer, the same workspace cap.  One launch resamples Y of the
 * in-plane part of every cell straight from the packed integer frame (one dword per source sample), one replicates the plane's
 * border, the unchanged layer kernels run over the atlas (with the second replicate before layer 3), and one launch resamples
 * U, V (and A) of every item tile by tile of its chroma grid from the packed frame, saturates them, puts them beside Y' of the
 * item's cell, encodes and stores -- a packed row mixes luma and chroma, so one kernel writes both: six launches per atlas,
 * whatever n is.  A SINGLE item runs as srcnn_yuv_packed_upscale_rect_dev does, with its bands and its
 * SRCNN_YUV_PACKED_RECT_UNFUSED.  An item is single when the Y list would run its luma rect single (the mode is not strict, an
 * axis keeps its size or shrinks, the tile resampler does not serve its window, its cell has SRCNN_RECT_LIST_SINGLE_SAMPLES
 * samples or more or exceeds the workspace cap alone), when the CHROMA grid does not grow in both axes (ceil(w / 2) columns can
 * keep their number while w grows: a 4:2:2 format with w = 1 at 2x) or the tile resampler does not serve the chroma filter's
 * tables over the item's chroma columns and rows (at a tile width of 60 chroma columns for v210), when the stream is being
 * captured by the caller, or when SRCNN_YUV_PACKED_RECT_LIST_UNFUSED=1 is set.  srcnn_yuv_packed_upscale_rect_list_plan reports
 * the route without a device.
 *
 * Memory.  src and src_pitch describe the WHOLE w x h frame, as for srcnn_yuv_packed_upscale_rect_dev.  With (off, n) = the span
 * of pixels [x0, x0 + rw) of a dw-pixel row (srcnn_yuv_packed_span_bytes), an item's dst receives the byte at `off` of row y0
 * first: rh row segments of exactly n bytes.  A caller that repaints inside a full-size packed dw x dh surface passes
 * surface + y0 * pitch + off and the surface's pitch.  Pitches are in BYTES, 0 = tight (the tight row of the frame for the
 * source, n for an item); a non-zero pitch is at least that.  Every base and every non-zero pitch is a multiple of the format's
 * alignment (1, 2 or 4: srcnn_yuv_packed_row_bytes); a destination whose base and pitch are multiples of 16 takes a faster store
 * path, item by item.  `items` is a HOST array of n entries of item_size = sizeof(srcnn_yuv_packed_rect_item) bytes; it is read
 * completely before the call returns.
 *
 * Overlap.  Rects may overlap each other.  Items whose DESTINATION bytes overlap are the caller's business: where two items
 * write the same bytes of the output (a repaint inside one full-size surface), both write the whole frame's bytes there.
 *
 * Source rectangle.  No byte of the source is read outside the union of the items' srcnn_yuv_packed_rect_source rectangles,
 * each taken as the span of its columns (srcnn_yuv_packed_span_bytes on a w-pixel row) in its rows.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call.  Calls queued back to back need no synchronisation in between.
 *
 * Scratch comes from that stream's grow-only workspace, stays there until srcnn_trim, and scales with the atlas, never with
 * w * h or dw * dh: no float plane of the source frame exists on the batched route.  It is
 *     136 B per sample of the largest atlas (the 32 layer-2 planes, the upscaled Y plane, the layer-3 result),
 *     144 B per batched item (80 B for its cell, 64 B for its destination) and 144 B per atlas (the closing entry of both tables),
 * which is what the plan's scratch_bytes states; single items keep what include/srcnn_amd_yuv_packed_rect.h states for them.
 * The atlases of one call hold at most the workspace cap (srcnn_set_workspace_limit) in layer-2 planes each and run one after
 * another out of the same scratch.
 *
 * Errors.  Everything is checked before any device lookup and before any work: all or nothing.  First the list itself, then
 * the frame in the order of srcnn_yuv_packed_upscale_rect_dev, then every item with that call's per-rect rules in its order;
 * srcnn_last_error starts with "item K: " for the first offending index.
 *   SRCNN_E_ARG          item_size != sizeof(srcnn_yuv_packed_rect_item), plan->struct_size != sizeof(srcnn_rect_list_plan),
 *                        NULL plan
 *   SRCNN_OK             n == 0 (nothing is done and nothing else is looked at; no device is needed)
 *   SRCNN_E_ARG          NULL items with n > 0
 *   SRCNN_E_UNSUPPORTED  n > 65536
 *   SRCNN_E_ARG          unknown format; NULL src, unknown filter, zero w / h
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^23 - 1 output columns, 2^31 - 1 pixels)
 *   SRCNN_E_ARG          a source pitch below the tight row, a source base address or pitch that is not a multiple of the
 *                        format's alignment
 *   SRCNN_E_ARG          per item: a NULL dst, zero rw / rh, a rect that is not inside dw x dh (x0 + rw and y0 + rh are taken
 *                        without 32-bit wrap); then a rect that breaks the unit rule; then a pitch below n, a base address or
 *                        pitch that is not a multiple of the format's alignment; then source and destination byte ranges that
 *                        overlap (the range of a side is pitch * (rows - 1) + its row bytes)
 *   SRCNN_E_NODEVICE     no gfx950 device (the device call only)
 * The plan call checks the list, the format, the frame's geometry and an item's rect (inside, unit rule) only: no address or
 * pitch is looked at.  A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_YUV_PACKED_RECT_LIST_H
#define SRCNN_AMD_YUV_PACKED_RECT_LIST_H

#include <stddef.h>

#include "srcnn_amd_rect_list.h"
#include "srcnn_amd_yuv_packed_rect.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_YUV_PACKED_RECT_LIST_VERSION 1

typedef struct srcnn_yuv_packed_rect_item {
    unsigned x0, y0, rw, rh;        /* luma output coordinates inside dw x dh, under the unit rule of srcnn_amd_yuv_packed_rect.h */
    void*    dst;                   /* the byte at `off` of row y0 first: rh row segments of n bytes (srcnn_yuv_packed_span_bytes) */
    size_t   dst_pitch;             /* bytes; 0 = tight (n) */
} srcnn_yuv_packed_rect_item;       /* 32 bytes on LP64 */

int srcnn_yuv_packed_rect_list_abi_version(void);   /* SRCNN_AMD_YUV_PACKED_RECT_LIST_VERSION of the loaded library */
/* pure, no device: how srcnn_yuv_packed_upscale_rect_list_dev routes and packs this list at the current mode, workspace limit
 * and switches (a stream under capture, which only the call can see, sends every item the single way). */
int srcnn_yuv_packed_upscale_rect_list_plan(int format, unsigned w, unsigned h, float multiply, int filter,
                                            const srcnn_yuv_packed_rect_item* items, unsigned n, unsigned item_size,
                                            srcnn_rect_list_plan* plan);
int srcnn_yuv_packed_upscale_rect_list_dev(int format, unsigned w, unsigned h, float multiply, int filter,
                                           const void* src, size_t src_pitch,            /* the WHOLE w x h frame */
                                           const srcnn_yuv_packed_rect_item* items, unsigned n, unsigned item_size, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_YUV_PACKED_RECT_LIST_H */
