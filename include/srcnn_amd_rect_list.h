/*
 * srcnn_amd_rect_list.h -- A LIST OF RECTANGLES of the Y path's output in one call (the dirty rectangles of a frame, the
 * tiles of a viewport), device-resident: srcnn_y_path_rect_f32_dev (include/srcnn_amd_rect.h) for many rects at the launch
 * cost of a few.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside the rect extension headers, with a version of its own: the
 * functions declared here are listed in include/srcnn_amd_rect_list.abi, and tests/test_rect_list_abi.py holds header, list,
 * binding and the library's export table to each other.  The older headers are unchanged.
 *
 * Result.  After the call item k holds exactly what
 *     srcnn_y_path_rect_f32_dev(d_in, in_pitch, w, h, dw, dh, filter, x0, y0, rw, rh, d_out, out_pitch, stream)
 * would have written, at the current numerics mode (srcnn_set_mode): in SRCNN_MODE_STRICT bit for bit -- i.e. the samples of
 * the whole frame -- and in the other modes by construction, because there the list runs that call item by item.  Bytes between
 * a row's rw floats and the pitch are never written.
 *
 * How.  A pixel's arithmetic does not depend on where its tile lies, so the windows of many rects can share one launch of each
 * layer kernel.  A BATCHED item gets a cell of (rw + 12) x (rh + 12) samples in a scratch image, the atlas: the rect and a halo
 * of 6 (2 for the 5x5 layer, 4 for the 9x9 layer).  One launch resamples the in-plane part of every cell, one replicates the
 * plane's border into the out-of-plane part, the unchanged layer kernels run over the atlas as over a frame of its own (with a
 * second replicate, of the layer-2 activations, before layer 3: that layer clamps activations to the edge), and one launch
 * stores every rect where its item points: six launches per atlas, whatever n is.  A SINGLE item runs as the single call does.
 * An item is single when the mode is not strict, an axis keeps its size or shrinks, the tile resampler does not serve its
 * window, its cell has SRCNN_RECT_LIST_SINGLE_SAMPLES samples or more (2^21 unless the environment says otherwise: about a
 * 1436 x 1436 rect) or exceeds the workspace cap alone, the stream is being captured by the caller, or
 * SRCNN_RECT_LIST_UNFUSED=1 is set.  srcnn_y_path_rect_list_plan reports the route without a device.
 *
 * Memory.  As for the single call: d_in is the WHOLE source plane, pitches are in BYTES with 0 = tight, a non-zero pitch is a
 * multiple of 4 and at least the tight row, pointers are 4-byte aligned, all device memory of the call's context.  `items` is a
 * HOST array of n entries of item_size = sizeof(srcnn_rect_item) bytes; it is read completely before the call returns.
 * Rects may overlap each other.  Items whose DESTINATION bytes overlap are the caller's business: when both write the same
 * output sample there (a repaint inside one full-size plane), the bytes are simply equal.
 *
 * Source rectangle.  No byte of d_in is read outside the union of the items' srcnn_y_path_rect_source rectangles.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call.  Calls queued back to back need no synchronisation in between.
 *
 * Scratch comes from that stream's grow-only workspace and stays there until srcnn_trim: 136 B per sample of the largest atlas
 * (the 32 layer-2 planes, the upscaled plane, the result) and 80 B per batched item, which is what the plan's scratch_bytes
 * states; single items keep what srcnn_amd_rect.h states for them.  The atlases of one call hold at most the workspace cap
 * (srcnn_set_workspace_limit) in layer-2 planes each and run one after another out of the same scratch.
 *
 * Errors.  Every item is checked before any device lookup and before any work: all or nothing.  srcnn_last_error names the
 * first offending index.
 *   SRCNN_OK             n == 0 (nothing is done)
 *   SRCNN_E_ARG          item_size != sizeof(srcnn_rect_item), plan->struct_size != sizeof(srcnn_rect_list_plan), NULL items
 *                        with n > 0, NULL plan, NULL d_in; per item the rules of srcnn_y_path_rect_f32_dev (the plan call
 *                        checks an item's geometry only: d_out and out_pitch are not looked at)
 *   SRCNN_E_SCALE        dw or dh is zero
 *   SRCNN_E_UNSUPPORTED  n > 65536; sizes beyond the Y path's limits
 *   SRCNN_E_NODEVICE     no gfx950 device (the device call only)
 * A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_RECT_LIST_H
#define SRCNN_AMD_RECT_LIST_H

#include <stddef.h>

#include "srcnn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_RECT_LIST_VERSION 1

typedef struct srcnn_rect_item {
    unsigned x0, y0, rw, rh;  /* the rect, inside dw x dh */
    float*   d_out;           /* receives sample (x0, y0) at its first float; device memory of the call's context */
    size_t   out_pitch;       /* bytes; 0 = tight (4 * rw); else a multiple of 4, >= 4 * rw */
} srcnn_rect_item;

typedef struct srcnn_rect_list_plan {
    unsigned struct_size;                      /* sizeof(srcnn_rect_list_plan), set by the caller */
    unsigned batched_items, single_items;      /* how the call will route the items */
    unsigned atlases;                          /* passes of the batched route (workspace cap) */
    unsigned long long cell_samples, atlas_samples;   /* sum of (rw+12)*(rh+12) over batched items; sum of atlas areas */
    unsigned long long scratch_bytes;          /* what the batched route retains in the stream's workspace */
} srcnn_rect_list_plan;

int srcnn_rect_list_abi_version(void);   /* SRCNN_AMD_RECT_LIST_VERSION of the loaded library */
/* pure, no device: how srcnn_y_path_rect_list_f32_dev routes and packs this list at the current mode, workspace limit and
 * switches (a stream under capture, which only the call can see, sends every item the single way). */
int srcnn_y_path_rect_list_plan(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                                const srcnn_rect_item* items, unsigned n, unsigned item_size, srcnn_rect_list_plan* plan);
int srcnn_y_path_rect_list_f32_dev(const float* d_in, size_t in_pitch, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                                   const srcnn_rect_item* items, unsigned n, unsigned item_size, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_RECT_LIST_H */
