/*
 * srcnn_amd_yuv_packed.h -- PACKED YUV frames (YUY2, UYVY, YVYU, Y210 / Y212 / Y216, AYUV, Y410, Y416, v210) through the
 * SRCNN path, device-resident: what capture cards, SDI bridges and webcams deliver, without a de-interleave pass of the
 * caller's own around the planar call.
 *
 * A fourth EXTENSION of the stable ABI (include/srcnn_amd.h) beside include/srcnn_amd_yuv.h, include/srcnn_amd_yuv_ex.h and
 * include/srcnn_amd_rgb.h, with a version of its own: the functions declared here are listed in
 * include/srcnn_amd_yuv_packed.abi, and tests/test_yuv_packed_abi.py holds header, list, binding and the library's export
 * table to each other.  The other headers are unchanged.
 *
 * The call is srcnn_yuv_upscale_dev (include/srcnn_amd_yuv_ex.h) on another memory layout: Y goes through SRCNN with the
 * configured filter, chroma and alpha go through the chroma filter (box for SRCNN_FILTER_NEAREST, bilinear for every other
 * filter).  Input and output have the same format.
 *
 * Geometry.  Luma (and alpha) go from w x h to dw x dh, where srcnn_output_size(w, h, multiply, 0, &dw, &dh) gives the output
 * size.  4:2:2 formats carry ceil(w/2) x h chroma samples in and ceil(dw/2) x dh out, 4:4:4 formats w x h and dw x dh.  Odd
 * sizes are legal.  A frame is ONE plane of h rows; srcnn_yuv_packed_row_bytes gives the tight byte length of a row and the
 * alignment (1, 2 or 4) the base address and every non-zero pitch must have.
 *
 * Formats.  Memory order is low address first; words are little-endian.
 *   SRCNN_YUVP_YUY2              4:2:2,  8 bit   bytes Y0 U Y1 V per pixel pair                  4 * ceil(w/2) B   align 1
 *   SRCNN_YUVP_UYVY              4:2:2,  8 bit   bytes U Y0 V Y1                                 4 * ceil(w/2) B   align 1
 *   SRCNN_YUVP_YVYU              4:2:2,  8 bit   bytes Y0 V Y1 U                                 4 * ceil(w/2) B   align 1
 *   SRCNN_YUVP_Y210/_Y212/_Y216  4:2:2, 10 / 12 / 16 bit   16-bit words Y0 U Y1 V, the value in the high `depth` bits
 *                                                                                                8 * ceil(w/2) B   align 2
 *   SRCNN_YUVP_VUYA              4:4:4 + alpha,  8 bit   bytes V U Y A per pixel (Microsoft AYUV)          4 * w B   align 1
 *   SRCNN_YUVP_Y410              4:4:4 + alpha, 10 bit (alpha: 2 bit)   one 32-bit word per pixel: U bits 0-9, Y 10-19,
 *                                V 20-29, A 30-31                                                          4 * w B   align 4
 *   SRCNN_YUVP_Y416              4:4:4 + alpha, 16 bit   16-bit words U Y V A per pixel                     8 * w B   align 2
 *   SRCNN_YUVP_V210              4:2:2, 10 bit   six pixels in four 32-bit words, three 10-bit fields each at bits 0-9,
 *                                10-19, 20-29:  word 0 = Cb0 Y0 Cr0,  word 1 = Y1 Cb1 Y2,  word 2 = Cr1 Y3 Cb2,
 *                                word 3 = Y4 Cr2 Y5;  rows are whole 128-byte blocks of 48 pixels   128 * ceil(w/48) B   align 4
 *
 * Pitches are in BYTES.  A pitch of 0 means tight rows.  A non-zero pitch must be at least the tight row and a multiple of
 * the format's alignment, as the base address must be.  Bytes between the tight row and the pitch are never written.
 *
 * Values.  The Y, U and V samples of the result are, sample for sample, what srcnn_yuv_upscale_dev produces for the
 * SRCNN_YUV_PLANAR frame of the same chroma format and depth that holds the same samples (Y21x: msb_aligned = 1).  With
 * s = depth - 8 and maxv = 2^depth - 1:
 *   Reading: only the bits of a field count.  Stray bits beside it are ignored: the low 16 - depth bits of a Y21x word,
 *        bits 30-31 of a v210 word.
 *   Y' = (unsigned) (Yf * 2^s), where Yf is the float Y path (srcnn_y_path_f32_dev) of the plane (float)Y * 2^-s with
 *        `filter`, at the current numerics mode.  Both scalings are exact in fp32.  Layer 3 clamps Yf to [0, 255], so
 *        Y' <= 255 * 2^s (1020 at 10 bits): the ceiling the reference puts on 8-bit data, expressed at the higher depth.
 *   U', V' = to_uN(resample((float)U)) on the native scale (no division), with the chroma filter, as
 *        srcnn_resample_f32_dev computes it; to_uN is MIN(maxv, x), then MAX(0, x), then truncation.  A chroma plane whose
 *        size does not change is copied sample for sample.
 *   A' = to_uN(resample((float)A)) on alpha's own scale with the chroma filter: N = 8 (VUYA), 2 (Y410) or 16 (Y416).  An
 *        alpha plane whose size does not change is copied.
 *   Slots of a tight row that carry no sample are ignored on input and written as ZERO: the second Y of the last pair at
 *        odd w, the v210 fields beyond w luma and ceil(w/2) chroma samples up to the end of the row's last 128-byte block,
 *        bits 30-31 of every v210 word, the low 16 - depth bits of every Y21x word.
 *
 * Stream.  Asynchronous on `stream`, like every *_dev call: it runs on the stream's context (srcnn_stream_create), or on
 * the calling thread's current context for NULL or a raw HIP stream.  Scratch comes from that stream's grow-only
 * workspace and stays there until srcnn_trim.  Retained bytes: 4 * (p * w*h + (p - 1) * dw*dh + dw*band) for the float
 * planes of the call -- p = 2 planes' worth for 4:2:2 (Y, and U + V of half the width each), 4 for 4:4:4 + alpha; band: the
 * Y' rows of one pass -- beside the Y path's own 132 B per output pixel of a band.  At 2x with one band that is 10 + 132
 * (4:2:2) or 20 + 132 (4:4:4 + alpha) B per output pixel.  band = dh unless the layer-2 planes of the frame exceed the workspace cap
 * (srcnn_set_workspace_limit): then Y is produced in horizontal bands, with identical bytes.
 *
 * Errors (validation comes before any device lookup):
 *   SRCNN_E_ARG          unknown format, NULL pointer, zero size, unknown filter, a pitch below the tight row, a base address
 *                        or pitch that is not a multiple of the format's alignment, or source and destination byte ranges
 *                        that overlap
 *   SRCNN_E_SCALE        `multiply` gives a zero output size
 *   SRCNN_E_UNSUPPORTED  sizes beyond the Y path's limits (2^20 rows, 2^31 - 1 pixels)
 *   SRCNN_E_NODEVICE     no gfx950 device
 */
#ifndef SRCNN_AMD_YUV_PACKED_H
#define SRCNN_AMD_YUV_PACKED_H

#include <stddef.h>

#include "srcnn_amd.h"

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SRCNN_AMD_YUV_PACKED_VERSION 1
#define SRCNN_YUVP_YUY2 0   /* 4:2:2  8 bit: Y0 U Y1 V */
#define SRCNN_YUVP_UYVY 1   /* 4:2:2  8 bit: U Y0 V Y1 */
#define SRCNN_YUVP_YVYU 2   /* 4:2:2  8 bit: Y0 V Y1 U */
#define SRCNN_YUVP_Y210 3   /* 4:2:2 10 bit: words Y0 U Y1 V, high bits */
#define SRCNN_YUVP_Y212 4   /* 4:2:2 12 bit: the same */
#define SRCNN_YUVP_Y216 5   /* 4:2:2 16 bit: the same */
#define SRCNN_YUVP_VUYA 6   /* 4:4:4 + alpha  8 bit: V U Y A */
#define SRCNN_YUVP_Y410 7   /* 4:4:4 + alpha 10 bit (alpha 2): U | Y << 10 | V << 20 | A << 30 */
#define SRCNN_YUVP_Y416 8   /* 4:4:4 + alpha 16 bit: words U Y V A */
#define SRCNN_YUVP_V210 9   /* 4:2:2 10 bit: 6 pixels in 4 words, rows of 128-byte blocks */

int srcnn_yuv_packed_abi_version(void);   /* SRCNN_AMD_YUV_PACKED_VERSION of the loaded library */
/* pure, no device: tight row bytes of a w-pixel row, and the alignment (1, 2 or 4) that the base address and a non-zero
 * pitch need.  Either of row_bytes / alignment may be NULL. */
int srcnn_yuv_packed_row_bytes(int format, unsigned w, size_t* row_bytes, unsigned* alignment);
int srcnn_yuv_packed_upscale_dev(int format, unsigned w, unsigned h, float multiply, int filter,
                                 const void* src, size_t src_pitch, void* dst, size_t dst_pitch, void* stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SRCNN_AMD_YUV_PACKED_H */
