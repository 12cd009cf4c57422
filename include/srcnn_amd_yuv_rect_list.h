/*
 * srcnn_amd_yuv_rect_list.h -- A LIST OF RECTANGLES of a planar or semi-planar YUV frame's output in one call (the dirty
 * rectangles of a video surface in a compositor or a screen-content transcoder), device-resident: srcnn_yuv_upscale_rect_dev
 * (include/srcnn_amd_yuv_rect.h) for many rects at the launch cost of a few, built on the atlas of
 * include/srcnn_amd_rect_list.h.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_yuv_rect.h, include/srcnn_amd_rect_list.h and
 * include/srcnn_amd_rgb_rect_list.h, with a version of its own: the functions declared here are listed in
 * include/srcnn_amd_yuv_rect_list.abi, and tests/test_yuv_rect_list_abi.py holds header, list, binding and the library's export
 * table to each other.  The older headers are unchanged.  Packed formats (include/srcnn_amd_yuv_packed_rect.h) are not served here.
 *
 * Result.  After the call item k holds exactly what
 *     srcnn_yuv_upscale_rect_dev(fmt, w, h, multiply, filter, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, stream)
 * would have written for that item's rect and dst, at the current numerics mode (srcnn_set_mode): in SRCNN_MODE_STRICT byte
 * for byte, the zero bits beside the value included -- i.e. every item is a crop of what srcnn_yuv_upscale_dev writes for the
 * whole frame -- and in the other modes by construction, because there the list runs that call item by item.  Bytes outside
 * an item's row segments (rw luma samples, the chroma rect's columns) are never written.  Formats, planes, the chroma rect, the
 * alignment of x0 / y0 and every value formula are those of include/srcnn_amd_yuv_rect.h.
 *
 * How.  A BATCHED item shares the layer kernels' launches with the others through the atlas of include/srcnn_amd_rect_list.h:
 * the same cells of (rw + 12) x (rh + 12) samples, the same packer, the same workspace cap.  One launch resamples Y of the
 * in-plane part of every cell straight from the integer luma plane, one replicates the plane's border, the unchanged layer
 * kernels run over the atlas (with the second replicate before layer 3), one launch writes Y' of every rect into its luma plane
 * in the caller's format, and one resamples U and V of every item's chroma rect tile by tile from the integer chroma plane(s)
 * and stores them: seven launches per atlas, whatever n is.  A SINGLE item runs as srcnn_yuv_upscale_rect_dev does, with its
 * bands and its SRCNN_YUV_RECT_UNFUSED.  An item is single when the Y list would run its luma rect single (the mode is not
 * strict, an axis keeps its size or shrinks, the tile resampler does not serve its window, its cell has
 * SRCNN_RECT_LIST_SINGLE_SAMPLES samples or more or exceeds the workspace cap alone), when the CHROMA grid does not grow in both
 * axes (ceil(w / 2) columns can keep their number while w grows: w = 1 at 2x, or 4:2:0 with w = 3 at 4/3) or the tile resampler
 * does not serve the chroma filter's tables over the item's chroma rect, when the stream is being captured by the caller, or
 * when SRCNN_YUV_RECT_LIST_UNFUSED=1 is set.  srcnn_yuv_upscale_rect_list_plan reports the route without a device.
 *
 * Memory.  src and src_pitch describe the WHOLE w x h frame, as for srcnn_yuv_upscale_rect_dev.  An item's dst are the planes of
 * an rw x rh frame in fmt: dst[0] receives luma sample (x0, y0) first, dst[1] and dst[2] chroma sample (x0 / 2, y0 / 2) first
 * (each axis under its own subsampling; a UV plane that U, V pair; dst[2] of a semi-planar format is not looked at).  A caller
 * that repaints inside a full-size dw x dh surface passes the addresses of those samples and the surface's pitches.  Pitches are
 * in BYTES, 0 = tight rows (of the frame for the source, of the rect for an item); a non-zero pitch is at least the row.  At
 * depth 8 bases need no alignment (bases and pitches that are multiples of 4 -- 8 for a UV plane -- take a faster store path,
 * item by item and per plane kind); above 8 every base address and every non-zero pitch is even (multiples of 8 -- 16 for a UV
 * plane -- take the faster path).  `items` is a HOST array of n entries of item_size = sizeof(srcnn_yuv_rect_item) bytes; it is
 * read completely before the call returns.
 *
 * Overlap.  Rects may overlap each other.  Items whose DESTINATION bytes overlap are the caller's business: where two items
 * write the same output sample (a repaint inside one full-size surface), the bytes are simply equal.  That covers two
 * neighbouring rects that share a chroma column or row: an odd-width rect that does not reach the right border writes the
 * chroma column its last luma column lies in, and so does any rect of the same surface that holds the other luma column of
 * that chroma sample -- both write the whole frame's value.
 *
 * Source rectangle.  No byte of a source plane is read outside the union, per plane, of the items' srcnn_yuv_rect_source
 * rectangles.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call.  Calls queued back to back need no synchronisation in between.
 *
 * Scratch comes from that stream's grow-only workspace, stays there until srcnn_trim, and scales with the atlas, never with
 * w * h or dw * dh: no float plane of the source frame exists on the batched route.  It is
 *     136 B per sample of the largest atlas (the 32 layer-2 planes, the upscaled Y plane, the layer-3 result),
 *     160 B per batched item (80 B for its cell, 80 B for its destinations) and 160 B per atlas (the closing entry of both tables),
 * which is what the plan's scratch_bytes states; single items keep what include/srcnn_amd_yuv_rect.h states for them.  The
 * atlases of one call hold at most the workspace cap (srcnn_set_workspace_limit) in layer-2 planes each and run one after
 * another out of the same scratch.
 *
 * Errors.  Everything is checked before any device lookup and before any work: all or nothing.  First the list itself, then
 * the frame in the order of srcnn_yuv_upscale_rect_dev, then every item with that call's per-rect rules in its order;
 * srcnn_last_error starts with "item K: " for the first offending index.
 *   SRCNN_E_ARG          item_size != sizeof(srcnn_yuv_rect_item), plan->struct_size != sizeof(srcnn_rect_list_plan), NULL plan
 *   SRCNN_OK             n == 0 (nothing is done and nothing else is looked at; no device is needed)
 *   SRCNN_E_ARG          NULL items with n > 0
 *   SRCNN_E_UNSUPPORTED  n > 65536
 *   SRCNN_E_ARG          NULL fmt, struct_size other than sizeof(srcnn_yuv_format), unknown layout / chroma / depth,
 *                        msb_aligned other than 0 / 1 or set at depth 8; NULL source plane array or required source plane,
 *                        unknown filter, zero w / h
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^23 - 1 output columns, 2^31 - 1 pixels)
 *   SRCNN_E_ARG          a source pitch below its row, at depth > 8 an odd source base address or pitch
 *   SRCNN_E_ARG          per item: a NULL required destination plane, zero rw / rh, a rect that is not inside dw x dh (x0 + rw
 *                        and y0 + rh are taken without 32-bit wrap); then an odd x0 (4:2:0, 4:2:2) or odd y0 (4:2:0); then a
 *                        pitch below its row, at depth > 8 an odd base address or odd pitch; then any source plane whose whole
 *                        byte range overlaps that of a destination plane of the item, or two destination planes of the item
 *                        that overlap each other
 *   SRCNN_E_NODEVICE     no gfx950 device (the device call only)
 * The plan call checks the list, the frame's format and geometry, and an item's geometry (rect and origin) only: no plane
 * address or pitch is looked at.  A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_YUV_RECT_LIST_H
#define SRCNN_AMD_YUV_RECT_LIST_H

#include <stddef.h>

#include "srcnn_amd_rect_list.h"
#include "srcnn_amd_yuv_rect.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_YUV_RECT_LIST_VERSION 1

typedef struct srcnn_yuv_rect_item {
    unsigned x0, y0, rw, rh;        /* luma output coordinates, inside dw x dh; alignment rules of srcnn_amd_yuv_rect.h */
    void*    dst[3];                /* the planes of an rw x rh frame in fmt: luma (x0, y0) first, chroma (x0/2, y0/2) first */
    size_t   dst_pitch[3];          /* bytes; 0 = tight rows of the rect */
} srcnn_yuv_rect_item;              /* 64 bytes on LP64 */

int srcnn_yuv_rect_list_abi_version(void);   /* SRCNN_AMD_YUV_RECT_LIST_VERSION of the loaded library */
/* pure, no device: how srcnn_yuv_upscale_rect_list_dev routes and packs this list at the current mode, workspace limit and
 * switches (a stream under capture, which only the call can see, sends every item the single way). */
int srcnn_yuv_upscale_rect_list_plan(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                     const srcnn_yuv_rect_item* items, unsigned n, unsigned item_size,
                                     srcnn_rect_list_plan* plan);
int srcnn_yuv_upscale_rect_list_dev(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                    const void* const src[3], const size_t src_pitch[3],   /* the WHOLE w x h frame */
                                    const srcnn_yuv_rect_item* items, unsigned n, unsigned item_size, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_YUV_RECT_LIST_H */
