/*
 * srcnn_amd_yuv.h -- 8-bit YUV 4:2:0 video frames (I420 / NV12) through the SRCNN path, device-resident.
 *
 * An EXTENSION of the stable ABI (include/srcnn_amd.h, frozen at SRCNN_AMD_ABI_VERSION 5) with a version of its own: the
 * functions declared here are listed in include/srcnn_amd_yuv.abi, and tests/test_yuv_abi.py holds header, list, binding
 * and the library's export table to each other.
 *
 * The call is a composition of pieces that are already bit-exact against the reference, in the form its colour shell uses
 * them for RGB (src/libsrcnn.cpp:665-726, :889-905): Y goes through SRCNN with the configured filter, the chroma planes go
 * through the chroma filter (box for SRCNN_FILTER_NEAREST, bilinear for every other filter), and the convolved Y is
 * truncated to 8 bits like the reference's conv-Y output.
 *
 * Geometry.  Luma goes from w x h to dw x dh, where srcnn_output_size(w, h, multiply, 0, &dw, &dh) gives the output size
 * (the reference's float truncation, as in ProcessSRCNN).  Chroma planes are ceil(w/2) x ceil(h/2) in and
 * ceil(dw/2) x ceil(dh/2) out.  Odd sizes are legal.
 *
 * Planes.  SRCNN_YUV_I420: plane[0] = Y, plane[1] = U, plane[2] = V.  SRCNN_YUV_NV12: plane[0] = Y, plane[1] = UV with U
 * first, interleaved; plane[2] is ignored.  All planes live in device memory of the call's context.
 *
 * Pitches are in bytes.  A pitch of 0 (or a NULL pitch array) means tight rows.  A non-zero pitch must be at least the
 * row's byte length: w for Y, ceil(w/2) for an I420 chroma row, 2*ceil(w/2) for an NV12 UV row (likewise for the
 * output with dw).  Base pointers need no alignment.  Padding bytes between rows are never written.
 *
 * Values.
 *   Y' = (unsigned char) Yf, where Yf is the float Y path (srcnn_y_path_f32_dev) of the plane (float)Y with `filter`, at
 *        the current numerics mode.  Layer 3 already clamps Yf to [0, 255]: the conversion truncates.
 *   U', V' = to_u8(resample((float)U)) with the chroma filter, as srcnn_resample_f32_dev computes it, where to_u8 is
 *        MIN(255, x), then MAX(0, x), then truncation.  A chroma plane whose size does not change is copied (the
 *        library's documented identity-size deviation from the reference's half copy).
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call: it runs on the stream's context (srcnn_stream_create), or on
 * the calling thread's current context for NULL or a raw HIP stream.  Scratch comes from that stream's grow-only
 * workspace and stays there until srcnn_trim.  Retained bytes: 4 * (w*h + 2*cw*ch + 2*dcw*dch + dw*band) for the float
 * planes of the call (cw x ch, dcw x dch: the chroma sizes above; band: the Y' rows of one pass), beside the Y path's
 * own 132 B per output pixel of a band (128 B of layer-2 planes + the upscaled Y, as srcnn_y_path_f32_dev).  At 2x
 * with one band that is 7.5 + 132 = about 140 B per output pixel (4.6 GB for a 7680x4320 output).  band = dh unless the
 * layer-2 planes of the frame exceed the workspace cap (srcnn_set_workspace_limit): then Y is produced in horizontal bands,
 * with identical bytes.
 *
 * Errors (validation comes before any device lookup):
 *   SRCNN_E_ARG          NULL plane, zero size, unknown format or filter, a pitch too small, or an input plane whose
 *                        byte range overlaps that of an output plane
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^31 - 1 pixels)
 *   SRCNN_E_NODEVICE     no gfx950 device
 */
#ifndef SRCNN_AMD_YUV_H
#define SRCNN_AMD_YUV_H

#include "srcnn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_YUV_VERSION 1
#define SRCNN_YUV_I420 0   /* planes Y, U, V */
#define SRCNN_YUV_NV12 1   /* planes Y, UV (U first, interleaved); plane[2] ignored */

int srcnn_yuv_abi_version(void);   /* SRCNN_AMD_YUV_VERSION of the loaded library */
int srcnn_yuv420_upscale_dev(int format, unsigned w, unsigned h, float multiply, int filter,
                             const unsigned char* const src[3], const size_t src_pitch[3],
                             unsigned char* const dst[3], const size_t dst_pitch[3], void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_YUV_H */
