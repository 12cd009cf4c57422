/*
 * srcnn_amd_rgb.h -- RGB(A) images that are already in device memory through the whole SRCNN pass (colour split, SRCNN on Y,
 * chroma resample, merge), device-resident: the device-side counterpart of srcnn_process_u8.
 *
 * A third EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_yuv.h and include/srcnn_amd_yuv_ex.h,
 * with a version of its own: the functions declared here are listed in include/srcnn_amd_rgb.abi, and tests/test_rgb_abi.py
 * holds header, list, binding and the library's export table to each other.  The three older headers are unchanged.
 *
 * Geometry.  The output is dw x dh, where srcnn_output_size(w, h, multiply, 0, &dw, &dh) gives the output size.  Input and
 * output have the same format.  srcnn_rgb_plane_size gives columns, rows and tight row bytes of every plane.
 *
 * Planes.  SRCNN_RGB_INTERLEAVED: plane[0] holds pixels of `channels` = 3 + alpha samples each, in the order R,G,B[,A]
 * (SRCNN_RGB_ORDER_RGB) or B,G,R[,A] (SRCNN_RGB_ORDER_BGR); plane[1..3] are ignored.  SRCNN_RGB_PLANAR: plane[0..2] = R, G, B
 * (SRCNN_RGB_ORDER_BGR: plane[0] = B, plane[2] = R), plane[3] = A when alpha is set and ignored otherwise -- a torch CHW
 * tensor.  All planes live in device memory of the call's context.
 *
 * Samples.  depth 8: one byte per sample.  depth 10 / 12 / 14 / 16: one little-endian 16-bit word per sample, the value in
 * its low bits.
 *
 * Pitches are in BYTES.  A pitch of 0 (or a NULL pitch array) means tight rows.  A non-zero pitch must be at least the
 * row's byte length.  At depth 8 base pointers need no alignment; above 8 every base address and every non-zero pitch must
 * be even.  Padding bytes between rows are never written.
 *
 * Values.  Let s = depth - 8, maxv = 2^depth - 1.
 *   Reading: a 16-bit sample is word & maxv (stray high bits are ignored).  R, G, B (and A) become floats as
 *        (float)v * 2^-s, which is exact.
 *   Arithmetic on those floats is exactly what srcnn_process_u8 does, in the same order and with the same roundings:
 *        Y  = (0.299 R) + (0.587 G) + (0.114 B),  Cb = 128 - (0.1687 R) - (0.3313 G) + (0.5 B),
 *        Cr = 128 + (0.5 R) - (0.4187 G) - (0.0813 B), every product and sum rounded to fp32 on its own;
 *        Y' = the float Y path (srcnn_y_path_f32_dev) of Y with `filter`, at the current numerics mode;
 *        Cb', Cr', A' = the planes resampled with the chroma filter (box for SRCNN_FILTER_NEAREST, bilinear for every other
 *        filter), as srcnn_resample_f32_dev computes it;
 *        R' = Y' + 45 (Cr' - 128) / 32,  G' = Y' - (11 (Cb' - 128) + 23 (Cr' - 128)) / 32,  B' = Y' + 113 (Cb' - 128) / 64.
 *   Writing: every sample is (unsigned)(clamp(v) * 2^s), where clamp is MIN(255.f, v) followed by MAX(0.f, v) in the
 *        reference's macro forms.  The largest code is therefore 255 * 2^s (1020 at 10 bits): the ceiling
 *        include/srcnn_amd_yuv_ex.h documents for Y'.  High bits of 16-bit outputs are zero.
 *   dst_conv (optional) receives (unsigned)(Y' * 2^s), one sample of the image's word size per pixel, dw x dh.
 *   depth == 8, SRCNN_RGB_ORDER_RGB, interleaved: the bytes of dst[0] and dst_conv are those of
 *        srcnn_process_u8(rgb, w, h, 3 + alpha, multiply, filter, out, conv) for every argument -- including the identity
 *        size, where no plane is resampled (the library's pinned identity-size deviation).  SRCNN_RGB_ORDER_BGR, the planar
 *        layout and pitches rearrange the same samples.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call: it runs on the stream's context (srcnn_stream_create), or on
 * the calling thread's current context for NULL or a raw HIP stream.  Scratch comes from that stream's grow-only workspace
 * and stays there until srcnn_trim.  Retained bytes, with c = 3 + alpha and band = the Y' rows of one pass:
 * 4 * c * (w*h + dw*band) for the float planes of the call, beside the Y path's own 132 B per output pixel of a band; at 2x
 * with one band that is 15 + 132 (RGB) or 20 + 132 (RGBA) B per output pixel.  The reference's own format -- depth 8,
 * interleaved, SRCNN_RGB_ORDER_RGB, tight rows on both sides, an up-scale in both axes -- is read and written by the fused
 * colour kernels srcnn_process_u8 uses: no float plane of source or destination size then exists, and the call keeps
 * 4 * dw * band = 4 + 132 B per output pixel.  Both routes give the same bytes.
 *
 * Bands.  band = dh unless the layer-2 planes of the frame exceed the workspace cap (srcnn_set_workspace_limit): then Y' is
 * produced in horizontal bands, with identical bytes.
 *
 * Errors (validation comes before any device lookup):
 *   SRCNN_E_ARG          NULL fmt, struct_size other than sizeof(srcnn_rgb_format), unknown layout / order / alpha / depth,
 *                        NULL required plane, zero size, unknown filter, a pitch too small, at depth > 8 an odd base address
 *                        or odd pitch, any input plane whose byte range overlaps that of an output plane (dst_conv counts
 *                        as an output plane), or two output planes that overlap each other
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^31 - 1 pixels)
 *   SRCNN_E_NODEVICE     no gfx950 device
 * A strict-only build exports the same set.
 */
#ifndef SRCNN_AMD_RGB_H
#define SRCNN_AMD_RGB_H

#include <stddef.h>

#include "srcnn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_RGB_VERSION 1
#define SRCNN_RGB_INTERLEAVED 0   /* plane[0] = pixels of `channels` samples each */
#define SRCNN_RGB_PLANAR      1   /* plane[0..2] = R, G, B; plane[3] = A when alpha (torch CHW) */
#define SRCNN_RGB_ORDER_RGB   0   /* interleaved sample order R,G,B[,A] */
#define SRCNN_RGB_ORDER_BGR   1   /* interleaved sample order B,G,R[,A]; planar: plane[0] = B, plane[2] = R */

typedef struct srcnn_rgb_format {
    unsigned struct_size;  /* sizeof(srcnn_rgb_format), anything else: SRCNN_E_ARG */
    int layout;            /* SRCNN_RGB_INTERLEAVED | SRCNN_RGB_PLANAR */
    int order;             /* SRCNN_RGB_ORDER_RGB | SRCNN_RGB_ORDER_BGR */
    int alpha;             /* 0: 3 channels, 1: 4 channels, alpha last */
    int depth;             /* 8: one byte per sample; 10/12/14/16: one little-endian 16-bit word, value in the low bits */
} srcnn_rgb_format;

int srcnn_rgb_abi_version(void);   /* SRCNN_AMD_RGB_VERSION of the loaded library */
/* pure, no device: columns, rows and tight row bytes of plane 0..3 of a w x h image in fmt (unused planes: 0 x 0).  Any of
 * cols / rows / row_bytes may be NULL. */
int srcnn_rgb_plane_size(const srcnn_rgb_format* fmt, unsigned w, unsigned h, int plane,
                         unsigned* cols, unsigned* rows, size_t* row_bytes);
int srcnn_rgb_upscale_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                          const void* const src[4], const size_t src_pitch[4],
                          void* const dst[4], const size_t dst_pitch[4],
                          void* dst_conv, size_t dst_conv_pitch,   /* optional truncated Y' plane, NULL: none */
                          void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_RGB_H */
