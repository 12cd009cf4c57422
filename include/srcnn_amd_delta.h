/*
 * srcnn_amd_delta.h -- UPSCALE ONLY WHAT CHANGED between two Y frames that are both in device memory: the library finds on the
 * device which tiles of the output can differ, and repaints those through the rect list call (include/srcnn_amd_rect_list.h)
 * inside the caller's full-size output plane.  For callers that hold last frame and this frame but no list of dirty
 * rectangles: remote desktops, screen capture, static-camera video, paused layers.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside the rect list extension, with a version of its own: the functions
 * declared here are listed in include/srcnn_amd_delta.abi, and tests/test_delta_abi.py holds header, list, binding and the
 * library's export table to each other.  The older headers are unchanged.
 *
 * The contract.  A grid of tile_w x tile_h output samples covers dw x dh: cols = ceil(dw / tile_w), rows = ceil(dh / tile_h),
 * the last column and row may be partial.  tile_w / tile_h: 0 = 64, otherwise 8 ... 65535.  Tile (c, r) is DIRTY if and only if
 * some source sample inside srcnn_y_path_rect_source(w, h, dw, dh, filter, <tile c,r>) has different 32-bit patterns in d_prev
 * and d_cur.  The comparison is on bit patterns: -0.0f against +0.0f is a difference, two NaNs with equal bits are not.  The
 * definition is exact, not merely conservative.  Bytes between a row's w floats and the pitch are never read.
 *
 * Result of srcnn_y_path_delta_f32_dev.  In SRCNN_MODE_STRICT: if d_out held the Y path (srcnn_y_path_f32_dev) of the previous
 * frame, it now holds the Y path of the current one, bit for bit -- an output tile whose source rectangle is bitwise unchanged
 * cannot change, so this is not an approximation.  Samples of clean tiles are not written at all, and neither are bytes between
 * a row's dw floats and out_pitch.  In the other modes a sample is either untouched or what srcnn_y_path_rect_f32_dev gives in
 * that mode.
 *
 * How.  One kernel reads every sample of both planes once (8 * w * h bytes) and sets a byte per dirty tile; the flags are copied
 * to the host; maximal runs of dirty tiles of a tile row that repeat in the next row are joined into rects
 * (srcnn_y_path_delta_rects is that rule); srcnn_y_path_rect_list_f32_dev repaints them.  The frame is repainted as the single
 * rect (0, 0, dw, dh) instead when every tile is dirty, when there are more than 65536 rects, or when the sum of
 * (rw + 12) * (rh + 12) over the rects reaches SRCNN_DELTA_WHOLE_PERMILLE / 1000 of dw * dh (environment, default 850, the
 * measured crossover; read when the library loads).  Either route gives the same bits.
 *
 * Stream.  srcnn_y_path_delta_flags_dev is asynchronous on `stream`, like every *_dev call (its first call with a new geometry
 * uploads the span tables with a blocking copy, as a first call with a new size uploads its resampling tables).
 * srcnn_y_path_delta_f32_dev BLOCKS THE HOST until the flags have arrived -- one synchronisation of `stream`, so everything
 * queued on it before has finished too -- and queues the upscale itself asynchronously.  On a stream that the caller is capturing
 * into a graph it returns SRCNN_E_UNSUPPORTED before anything is queued: a capture cannot wait.  srcnn_y_path_delta_flags_dev
 * can be captured once it has run with the same geometry on that stream outside a capture; otherwise SRCNN_E_UNSUPPORTED.
 *
 * Memory.  d_prev, d_cur: whole w x h planes; d_out: the whole dw x dh plane; d_flags: cols * rows bytes, row-major, each 0 or 1
 * after the call, no byte outside written.  Pitches are in BYTES with 0 = tight, a non-zero pitch is a multiple of 4 and at
 * least the tight row, pointers are 4-byte aligned, all device memory of the call's context.  Where both source bases and both
 * pitches are multiples of 16 the kernel reads 16 bytes per lane and plane at a time.  Scratch comes from the stream's grow-only
 * workspace and stays there until srcnn_trim: 8 * (cols + rows) bytes of tables, cols * rows flag bytes on the device and
 * page-locked on the host, and what the rect list call states for the rects.
 *
 * Errors, all before any device lookup:
 *   SRCNN_E_ARG          NULL d_cur, d_flags or d_out; zero w or h; bad filter; a tile side of 1 ... 7 or above 65535; a base or
 *                        pitch that breaks the rules above; d_out overlapping d_prev or d_cur; stats->struct_size !=
 *                        sizeof(srcnn_delta_stats); NULL cols, rows, n or (with cols * rows > 0) flags; items == NULL with
 *                        cap > 0; cap below the number of rects (*n is set)
 *   SRCNN_E_SCALE        dw or dh is zero
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits; more than 2048 tile columns or tile rows (the kernel holds both span
 *                        tables in LDS); a stream under the caller's capture (see Stream)
 *   SRCNN_E_NODEVICE     no gfx950 device (the device calls only)
 * A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_DELTA_H
#define SRCNN_AMD_DELTA_H

#include <stddef.h>

#include "srcnn_amd_rect_list.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_DELTA_VERSION 1

typedef struct srcnn_delta_stats {
    unsigned struct_size;              /* sizeof(srcnn_delta_stats), set by the caller */
    unsigned tiles, dirty_tiles;       /* cols * rows; how many of them were dirty */
    unsigned rects;                    /* rects the dirty tiles coalesced into (0: nothing was queued) */
    unsigned whole_frame;              /* 1: repainted as the single rect (0, 0, dw, dh) */
    unsigned long long cell_samples;   /* sum of (rw + 12) * (rh + 12) over those rects */
} srcnn_delta_stats;

int srcnn_delta_abi_version(void);   /* SRCNN_AMD_DELTA_VERSION of the loaded library */
/* pure, no device: checks the geometry and reports the tile grid with the defaults applied */
int srcnn_y_path_delta_grid(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h,
                            unsigned* cols, unsigned* rows);
/* the dirty flags of the grid, cols * rows bytes at d_flags.  d_prev == NULL: "no previous frame" -- all ones, d_cur is not read */
int srcnn_y_path_delta_flags_dev(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h,
                                 unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h, unsigned char* d_flags, void* stream);
/* pure host, the coalescer: HOST flags (non-zero = dirty) of a cols x rows grid of tile_w x tile_h tiles (both given, not 0) over
 * dw x dh into rects whose items point into the full-size plane d_out (may be NULL; out_pitch 0 = tight).  The rects are
 * pairwise disjoint, their union is exactly the dirty tiles clipped to dw x dh.  *n: their number; items == NULL with cap == 0
 * counts only.  It does not apply the whole-frame rule. */
int srcnn_y_path_delta_rects(const unsigned char* flags, unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h, unsigned dw,
                             unsigned dh, float* d_out, size_t out_pitch, srcnn_rect_item* items, unsigned cap, unsigned* n);
/* the whole operation.  d_prev == NULL: the whole frame.  stats may be NULL */
int srcnn_y_path_delta_f32_dev(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h,
                               unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h, float* d_out, size_t out_pitch,
                               void* stream, srcnn_delta_stats* stats);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_DELTA_H */
