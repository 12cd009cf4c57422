// srcnn_yuv.h -- internal interface of the 8-bit YUV 4:2:0 conversion kernels (srcnn_yuv.hip).  Not installed; the public
// surface is include/srcnn_amd_yuv.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace srcnn {

// Pitched u8 plane -> tight float plane(s).  nv12 = false: `w` samples per row -> d0.  nv12 = true: `w` interleaved
// (U, V) pairs per row -> d0 (U) and d1 (V).  Rows [0, rows).
void launch_yuv_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, bool nv12, float* d0, float* d1,
                       hipStream_t s);
// Tight float rows -> pitched u8 plane, rows [0, rows) of the source to destination rows [row0, row0 + rows).
// sat = false: (unsigned char) v (Y': layer 3 already clamps); sat = true: MIN(255), MAX(0), truncation (chroma).
// s1 != NULL: NV12, `w` pairs (s0[i], s1[i]) interleaved per row.
void launch_yuv_pack(const float* s0, const float* s1, unsigned w, unsigned rows, bool sat, unsigned char* dst, size_t pitch,
                     unsigned row0, hipStream_t s);

// ---- 16-bit words, 10 / 12 / 14 / 16 significant bits (srcnn_yuv16.hip; include/srcnn_amd_yuv_ex.h) ----
// How a sample of `depth` bits sits in its little-endian 16-bit word, and the exact luma scalings (s = depth - 8).
struct Yuv16Rule {
    unsigned rshift = 0;    // read: (word >> rshift) & mask
    unsigned mask = 0;      // maxv = 2^depth - 1
    unsigned lshift = 0;    // write: value << lshift
    float down = 1.f;       // 2^-s: Y sample -> the Y path's 8-bit scale
    float up = 1.f;         // 2^s:  Yf -> Y'
};
// Pitched u16 plane -> tight float plane(s), like launch_yuv_unpack (uv = interleaved U, V words -> d0, d1).  luma: the
// values are multiplied by f.down; chroma stays on the native scale.  Base and pitch must be even.
void launch_yuv16_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, bool uv, const Yuv16Rule& f,
                         bool luma, float* d0, float* d1, hipStream_t s);
// Tight float rows -> pitched u16 plane, like launch_yuv_pack.  sat = false: (unsigned)(v * f.up) (Y'); sat = true:
// MIN(maxv), MAX(0), truncation (chroma).  s1 != NULL: interleaved (s0[i], s1[i]) words, saturated.
void launch_yuv16_pack(const float* s0, const float* s1, unsigned w, unsigned rows, bool sat, const Yuv16Rule& f,
                       unsigned char* dst, size_t pitch, unsigned row0, hipStream_t s);

}  // namespace srcnn
