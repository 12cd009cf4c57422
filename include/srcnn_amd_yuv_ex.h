/*
 * srcnn_amd_yuv_ex.h -- YUV video frames of 8 / 10 / 12 / 14 / 16 bits in 4:2:0, 4:2:2 or 4:4:4, planar or semi-planar
 * (P010, P016, I010, I210, I444 10/12-bit, NV12, I420 ...), through the SRCNN path, device-resident.
 *
 * A second EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_yuv.h, with a version of its own:
 * the functions declared here are listed in include/srcnn_amd_yuv_ex.abi, and tests/test_yuv_ex_abi.py holds header, list,
 * binding and the library's export table to each other.  include/srcnn_amd_yuv.h is unchanged.
 *
 * The call is the composition of srcnn_yuv420_upscale_dev, generalised: Y goes through SRCNN with the configured filter,
 * the chroma planes go through the chroma filter (box for SRCNN_FILTER_NEAREST, bilinear for every other filter).  Input
 * and output have the same format.
 *
 * Geometry.  Luma goes from w x h to dw x dh, where srcnn_output_size(w, h, multiply, 0, &dw, &dh) gives the output size.
 * Chroma planes are cw x ch in and dcw x dch out: SRCNN_YUV_420 ceil(w/2) x ceil(h/2) and ceil(dw/2) x ceil(dh/2),
 * SRCNN_YUV_422 ceil(w/2) x h and ceil(dw/2) x dh, SRCNN_YUV_444 w x h and dw x dh.  Odd sizes are legal.
 * srcnn_yuv_plane_size gives columns, rows and tight row bytes of every plane.
 *
 * Planes.  SRCNN_YUV_PLANAR: plane[0] = Y, plane[1] = U, plane[2] = V.  SRCNN_YUV_SEMIPLANAR: plane[0] = Y, plane[1] = UV
 * with U first, interleaved; plane[2] is ignored.  All planes live in device memory of the call's context.
 *
 * Samples.  depth 8: one byte per sample.  depth 10 / 12 / 14 / 16: one little-endian 16-bit word per sample.
 *
 * Pitches are in BYTES.  A pitch of 0 (or a NULL pitch array) means tight rows.  A non-zero pitch must be at least the
 * row's byte length: cols at depth 8 and 2 * cols above, doubled again for a UV row.  At depth 8 base pointers need no
 * alignment; above 8 every base address and every non-zero pitch must be even.  Padding bytes between rows are never
 * written.
 *
 * Values.  Let s = depth - 8, maxv = 2^depth - 1.
 *   Reading a 16-bit sample: msb_aligned == 0: word & maxv (stray high bits are ignored); msb_aligned == 1:
 *        word >> (16 - depth) (stray low bits are ignored).
 *   Y' = (unsigned) (Yf * 2^s), where Yf is the float Y path (srcnn_y_path_f32_dev) of the plane (float)Y * 2^-s with
 *        `filter`, at the current numerics mode.  Both scalings are exact in fp32.  Layer 3 clamps Yf to [0, 255], so
 *        Y' <= 255 * 2^s (1020 at 10 bits): the top 2^s - 1 codes are never produced -- the ceiling the reference puts on
 *        8-bit data, expressed at the higher depth.  Narrow-range video (luma <= 940 at 10 bits) is not touched by it.
 *   U', V' = to_uN(resample((float)U)) on the native scale (no division), with the chroma filter, as
 *        srcnn_resample_f32_dev computes it; to_uN is MIN(maxv, x), then MAX(0, x), then truncation.  A chroma plane whose
 *        size does not change is copied sample for sample (after the read rule above).
 *   Writing: msb_aligned == 0: the value, high bits zero; msb_aligned == 1: value << (16 - depth), low bits zero.
 *   depth == 8, SRCNN_YUV_420: the same bytes as srcnn_yuv420_upscale_dev (planar = I420, semi-planar = NV12).
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call: it runs on the stream's context (srcnn_stream_create), or on
 * the calling thread's current context for NULL or a raw HIP stream.  Scratch comes from that stream's grow-only
 * workspace and stays there until srcnn_trim.  Retained bytes: 4 * (w*h + 2*cw*ch + 2*dcw*dch + dw*band) for the float
 * planes of the call (band: the Y' rows of one pass), beside the Y path's own 132 B per output pixel of a band.  At 2x
 * with one band that is 7.5 + 132 (4:2:0), 9 + 132 (4:2:2) or 12 + 132 (4:4:4) B per output pixel.  band = dh unless the
 * layer-2 planes of the frame exceed the workspace cap (srcnn_set_workspace_limit): then Y is produced in horizontal
 * bands, with identical bytes.
 *
 * Errors (validation comes before any device lookup):
 *   SRCNN_E_ARG          NULL fmt, struct_size other than sizeof(srcnn_yuv_format), unknown layout / chroma / depth,
 *                        msb_aligned not 0 / 1 or set at depth 8, NULL plane, zero size, unknown filter, a pitch too small,
 *                        at depth > 8 an odd base address or odd pitch, or an input plane whose byte range overlaps that
 *                        of an output plane
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^31 - 1 pixels)
 *   SRCNN_E_NODEVICE     no gfx950 device
 */
#ifndef SRCNN_AMD_YUV_EX_H
#define SRCNN_AMD_YUV_EX_H

#include <stddef.h>

#include "srcnn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_YUV_EX_VERSION 1
#define SRCNN_YUV_PLANAR     0   /* planes Y, U, V */
#define SRCNN_YUV_SEMIPLANAR 1   /* planes Y, UV (U first, interleaved); plane[2] ignored */
#define SRCNN_YUV_420 0          /* chroma ceil(w/2) x ceil(h/2) */
#define SRCNN_YUV_422 1          /* chroma ceil(w/2) x h        */
#define SRCNN_YUV_444 2          /* chroma w x h                */

typedef struct srcnn_yuv_format {
    unsigned struct_size;   /* sizeof(srcnn_yuv_format); anything else: SRCNN_E_ARG (room to grow) */
    int layout;             /* SRCNN_YUV_PLANAR | SRCNN_YUV_SEMIPLANAR */
    int chroma;             /* SRCNN_YUV_420 | _422 | _444 */
    int depth;              /* significant bits per sample: 8, 10, 12, 14 or 16.  8: one byte per sample.
                             * above 8: one little-endian 16-bit word per sample */
    int msb_aligned;        /* depth > 8 only.  0: value in the low `depth` bits (yuv420p10le, I010 ...).
                             * 1: value in the high `depth` bits (P010 / P012 / P016 / P210 / P410 ...) */
} srcnn_yuv_format;

int srcnn_yuv_ex_abi_version(void);   /* SRCNN_AMD_YUV_EX_VERSION of the loaded library */
/* pure, no device: sample columns, rows and tight row bytes of plane 0..2 of a w x h frame in `fmt` (a UV plane has one
 * column per U, V pair; plane 2 of a semi-planar frame is 0 x 0).  Any of cols / rows / row_bytes may be NULL. */
int srcnn_yuv_plane_size(const srcnn_yuv_format* fmt, unsigned w, unsigned h, int plane,
                         unsigned* cols, unsigned* rows, size_t* row_bytes);
int srcnn_yuv_upscale_dev(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                          const void* const src[3], const size_t src_pitch[3],
                          void* const dst[3], const size_t dst_pitch[3], void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_YUV_EX_H */
