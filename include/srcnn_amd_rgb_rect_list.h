/*
 * srcnn_amd_rgb_rect_list.h -- A LIST OF RECTANGLES of an RGB(A) image's output in one call (the dirty rectangles of a UI
 * surface, the tiles of a viewport), device-resident: srcnn_rgb_upscale_rect_dev (include/srcnn_amd_rgb_rect.h) for many rects
 * at the launch cost of a few, built on the atlas of include/srcnn_amd_rect_list.h.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_rgb_rect.h and include/srcnn_amd_rect_list.h,
 * with a version of its own: the functions declared here are listed in include/srcnn_amd_rgb_rect_list.abi, and
 * tests/test_rgb_rect_list_abi.py holds header, list, binding and the library's export table to each other.  The older headers
 * are unchanged.
 *
 * Result.  After the call item k holds exactly what
 *     srcnn_rgb_upscale_rect_dev(fmt, w, h, multiply, filter, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, dst_conv,
 *                                dst_conv_pitch, stream)
 * would have written for that item's rect, dst and dst_conv, at the current numerics mode (srcnn_set_mode): in
 * SRCNN_MODE_STRICT byte for byte -- i.e. every item is a crop of what srcnn_rgb_upscale_dev writes for the whole image --
 * and in the other modes by construction, because there the list runs that call item by item.  Bytes outside the rw pixels of
 * a row are never written.  Format, planes, samples and every value formula are those of include/srcnn_amd_rgb.h.
 *
 * How.  A BATCHED item shares the layer kernels' launches with the others through the atlas of include/srcnn_amd_rect_list.h:
 * the same cells of (rw + 12) x (rh + 12) samples, the same packer, the same workspace cap.  One launch resamples Y of the
 * in-plane part of every cell straight from the integer source pixels, one replicates the plane's border, the unchanged layer
 * kernels run over the atlas (with the second replicate before layer 3), and one launch resamples Cb, Cr (and A) of every rect
 * tile by tile from the integer source, merges them with Y' of the atlas and stores the pixels where the item points: six
 * launches per atlas, whatever n is.  A SINGLE item runs as srcnn_rgb_upscale_rect_dev does, with its bands and its
 * SRCNN_RGB_RECT_UNFUSED.  An item is single when the Y list would run it single (the mode is not strict, an axis keeps its
 * size or shrinks, the tile resampler does not serve its window, its cell has SRCNN_RECT_LIST_SINGLE_SAMPLES samples or more or
 * exceeds the workspace cap alone), when the tile resampler does not serve the chroma filter's tables over the rect, when the
 * stream is being captured by the caller, or when SRCNN_RGB_RECT_LIST_UNFUSED=1 is set.  srcnn_rgb_upscale_rect_list_plan
 * reports the route without a device.
 *
 * Memory.  src and src_pitch describe the WHOLE w x h image, as for srcnn_rgb_upscale_rect_dev.  An item's dst (and dst_conv)
 * is an rw x rh image in fmt with pixel (x0, y0) of the output first; a caller that repaints inside a full-size image passes
 * the address of that image's pixel (x0, y0) and the image's pitch.  Pitches are in BYTES, 0 = tight rows (of w pixels for the
 * source, of rw pixels for an item); a non-zero pitch is at least the row.  At depth 8 bases need no alignment (4-byte
 * aligned bases and pitches take a faster store path, item by item); above 8 every base address and every non-zero pitch is
 * even.  dst_conv is per item: NULL for none.  `items` is a HOST array of n entries of item_size =
 * sizeof(srcnn_rgb_rect_item) bytes; it is read completely before the call returns.  Rects may overlap each other.  Items
 * whose DESTINATION bytes overlap are the caller's business: where two items write the same output pixel (a repaint inside one
 * full-size image), the bytes are simply equal.
 *
 * Source rectangle.  No byte of any source plane is read outside the union of the items' srcnn_rgb_rect_source rectangles.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call.  Calls queued back to back need no synchronisation in between.
 *
 * Scratch comes from that stream's grow-only workspace, stays there until srcnn_trim, and scales with the atlas, never with
 * w * h or dw * dh: no float plane of the source image exists on the batched route.  It is
 *     136 B per sample of the largest atlas (the 32 layer-2 planes, the upscaled Y plane, the layer-3 result),
 *     168 B per batched item (80 B for its cell, 88 B for its destinations) and 80 B per atlas (the closing cell entry),
 * which is what the plan's scratch_bytes states; single items keep what include/srcnn_amd_rgb_rect.h states for them.  The
 * atlases of one call hold at most the workspace cap (srcnn_set_workspace_limit) in layer-2 planes each and run one after
 * another out of the same scratch.
 *
 * Errors.  Everything is checked before any device lookup and before any work: all or nothing.  First the list itself, then
 * the frame in the order of srcnn_rgb_upscale_rect_dev, then every item with that call's per-rect rules in its order;
 * srcnn_last_error starts with "item K: " for the first offending index.
 *   SRCNN_E_ARG          item_size != sizeof(srcnn_rgb_rect_item), plan->struct_size != sizeof(srcnn_rect_list_plan), NULL plan
 *   SRCNN_OK             n == 0 (nothing is done; no device is needed)
 *   SRCNN_E_ARG          NULL items with n > 0
 *   SRCNN_E_UNSUPPORTED  n > 65536
 *   SRCNN_E_ARG          NULL fmt, struct_size other than sizeof(srcnn_rgb_format), unknown layout / order / alpha / depth,
 *                        NULL source plane array or required source plane, unknown filter, zero w / h
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^23 - 1 output columns, 2^31 - 1 pixels)
 *   SRCNN_E_ARG          a source pitch below its row, at depth > 8 an odd source base address or pitch
 *   SRCNN_E_ARG          per item: a NULL required destination plane, zero rw / rh, a rect that is not inside dw x dh (x0 + rw
 *                        and y0 + rh are taken without 32-bit wrap); then a pitch below its row of rw pixels, at depth > 8 an
 *                        odd base address or odd pitch; then any source plane whose whole byte range overlaps that of a
 *                        destination plane of the item (dst_conv counts as one), or two destination planes of the item that
 *                        overlap each other
 *   SRCNN_E_NODEVICE     no gfx950 device (the device call only)
 * The plan call checks the list, the frame's format and geometry, and an item's geometry only: no plane address or pitch is
 * looked at.  A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_RGB_RECT_LIST_H
#define SRCNN_AMD_RGB_RECT_LIST_H

#include <stddef.h>

#include "srcnn_amd_rect_list.h"
#include "srcnn_amd_rgb_rect.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_RGB_RECT_LIST_VERSION 1

typedef struct srcnn_rgb_rect_item {
    unsigned x0, y0, rw, rh;        /* the rect, inside dw x dh */
    void*    dst[4];                /* an rw x rh image in fmt: pixel (x0, y0) first; planes as in srcnn_amd_rgb.h */
    size_t   dst_pitch[4];          /* bytes; 0 = tight rows of rw pixels */
    void*    dst_conv;              /* optional rw x rh truncated Y', NULL: none -- per item */
    size_t   dst_conv_pitch;
} srcnn_rgb_rect_item;              /* 96 bytes on LP64 */

int srcnn_rgb_rect_list_abi_version(void);   /* SRCNN_AMD_RGB_RECT_LIST_VERSION of the loaded library */
/* pure, no device: how srcnn_rgb_upscale_rect_list_dev routes and packs this list at the current mode, workspace limit and
 * switches (a stream under capture, which only the call can see, sends every item the single way). */
int srcnn_rgb_upscale_rect_list_plan(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                     const srcnn_rgb_rect_item* items, unsigned n, unsigned item_size,
                                     srcnn_rect_list_plan* plan);
int srcnn_rgb_upscale_rect_list_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                    const void* const src[4], const size_t src_pitch[4],   /* the WHOLE w x h source image */
                                    const srcnn_rgb_rect_item* items, unsigned n, unsigned item_size, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_RGB_RECT_LIST_H */
