/*
 * srcnn_amd_rect.h -- ONE RECTANGLE of the Y path's output (a viewport, a dirty rectangle, a tile) at the cost of that
 * rectangle, device-resident: the partial form of srcnn_y_path_f32_dev in both axes.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h) beside the YUV and RGB extension headers, with a version of its own: the
 * functions declared here are listed in include/srcnn_amd_rect.abi, and tests/test_rect_abi.py holds header, list, binding and
 * the library's export table to each other.  The older headers are unchanged.
 *
 * Result.  For a w x h float plane d_in and an output size dw x dh, sample (i, j) of the rw x rh result, i < rw, j < rh, is
 * sample (x0 + i, y0 + j) of what srcnn_y_path_f32_dev(d_in, w, h, dw, dh, filter, ...) computes at the current numerics mode
 * (srcnn_set_mode).  In SRCNN_MODE_STRICT it is that sample bit for bit, whatever the rect; the non-parity modes keep their
 * tolerances.
 *
 * How.  A pixel's arithmetic does not depend on where its tile lies.  The call resamples a WINDOW of the dw x dh plane --
 * the rect and a halo of 6 samples (2 for the 5x5 layer, 4 for the 9x9 layer), cut short at the borders of the plane -- and
 * runs the three layers on it as on a small frame; only the rect's samples are stored.  Work and scratch scale with the
 * window, not with dw: the window is Ww = min(dw, x0 + rw + 6) - max(0, x0 - 6) columns wide.
 *
 * Memory.  Both planes live in device memory of the call's context.  Pitches are in BYTES; 0 means tight rows (4 * w for
 * d_in, 4 * rw for d_out).  A non-zero pitch must be a multiple of 4 and at least the tight row; both pointers must be 4-byte
 * aligned.  d_in is the WHOLE source plane (row y at d_in + y * in_pitch); d_out receives sample (x0, y0) at its first
 * float.  Bytes between a row's rw floats and the pitch are never written.
 *
 * Source rectangle.  The result depends on no source sample outside the rectangle srcnn_y_path_rect_source reports (the
 * halo, then the first and last tap the resampler's contribution tables give for the window's columns and rows; an axis
 * that keeps its size is copied): a caller may have only that part of the source plane valid.  No other byte of d_in is read.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call: it runs on the stream's context (srcnn_stream_create), or on the
 * calling thread's current context for NULL or a raw HIP stream.
 *
 * Scratch comes from that stream's grow-only workspace and stays there until srcnn_trim.  With band = rh, or the rows of one
 * pass when the rect is banded (below), and src = the resampler's intermediate image (at most Ww * (source rows of the
 * band) or (source columns of the window) * (band + 12) floats), the call retains
 *     4 * Ww * (32 * (band + 4) + (band + 12) + band) + 4 * src   bytes,
 * i.e. about 136 B per sample of the window; SRCNN_MODE_FAST_F16 has no layer-2 planes and keeps 4 * Ww * (2 * band + 12) + 4 * src.
 *
 * Bands.  When the 32 layer-2 planes of the window, 32 * 4 * Ww * (rh + 4) bytes, exceed the workspace cap
 * (srcnn_set_workspace_limit), the rect is produced in horizontal bands, with identical bits.  A rect that spans the full
 * width of tight planes takes the path of srcnn_y_upscale2x_f32_band_dev.
 *
 * Errors (all before any device lookup):
 *   SRCNN_E_ARG          NULL d_in / d_out, zero w / h / rw / rh, a rect that is not inside dw x dh, unknown filter, a pitch
 *                        that is no multiple of 4 or below the tight row, a pointer that is not 4-byte aligned, input and
 *                        output byte ranges that overlap
 *   SRCNN_E_SCALE        dw or dh is zero
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^23 - 1 output columns, 2^31 - 1 source samples)
 *   SRCNN_E_NODEVICE     no gfx950 device
 * A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_RECT_H
#define SRCNN_AMD_RECT_H

#include <stddef.h>

#include "srcnn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_RECT_VERSION 1

int srcnn_rect_abi_version(void);   /* SRCNN_AMD_RECT_VERSION of the loaded library */
/* pure, no device: the source rectangle [*sx0, *sx0 + *sw) x [*sy0, *sy0 + *sh) the output rect depends on (halo + resampler
 * taps, read off the tables).  Same geometry errors as the call below.  Any of the four results may be NULL. */
int srcnn_y_path_rect_source(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                             unsigned x0, unsigned y0, unsigned rw, unsigned rh,
                             unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh);
int srcnn_y_path_rect_f32_dev(const float* d_in, size_t in_pitch, unsigned w, unsigned h,
                              unsigned dw, unsigned dh, int filter,
                              unsigned x0, unsigned y0, unsigned rw, unsigned rh,
                              float* d_out, size_t out_pitch, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_RECT_H */
