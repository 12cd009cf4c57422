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

// ---- packed frames: one plane that interleaves Y, U, V (and A) (srcnn_yuv_packed.hip; include/srcnn_amd_yuv_packed.h) ----
// The memory layouts the ten public formats come down to.  One lane of the kernels owns one 16-byte chunk of a packed row.
enum YuvPackedKind {
    kPk422x8 = 0,    // YUY2 / UYVY / YVYU: a dword per pixel pair, byte positions in sh[]          chunk: 8 Y, 4 U, 4 V
    kPk422x16,       // Y210 / Y212 / Y216: words Y0 U Y1 V, the value in the high bits             chunk: 4 Y, 2 U, 2 V
    kPk444x8,        // VUYA: a dword per pixel, byte positions in sh[]                             chunk: 4 Y, U, V, A
    kPk410,          // Y410: a dword per pixel, U | Y << 10 | V << 20 | A << 30                    chunk: 4 Y, U, V, A
    kPk444x16,       // Y416: words U Y V A                                                         chunk: 2 Y, U, V, A
    kPkV210,         // v210: 6 pixels in 4 dwords of three 10-bit fields                           chunk: 6 Y, 3 U, 3 V
};
struct YuvPackedRule {
    int kind = kPk422x8;
    unsigned sh[4] = {0, 0, 0, 0};   // 8-bit kinds: bit position inside the dword of Y0, U, Y1, V (4:2:2) or Y, U, V, A (4:4:4)
    unsigned shift = 0;              // kPk422x16: 16 - depth, read word >> shift, write value << shift
    unsigned mask = 255;             // maxv = 2^depth - 1 of Y, U, V
    unsigned amask = 0;              // maxv of alpha; 0: the format has none
    float down = 1.f, up = 1.f;      // 2^-s, 2^s (s = depth - 8): Y sample <-> the Y path's 8-bit scale
};
// Packed rows [0, rows) of `w` pixels -> tight float planes: dy (w per row, scaled by f.down), du / dv (ceil(w/2) per row for
// the 4:2:2 kinds, else w; native scale), da (w per row; only where f.amask).  Base and pitch must have the format's alignment.
void launch_yuvp_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, const YuvPackedRule& f, float* dy,
                        float* du, float* dv, float* da, hipStream_t s);
// Tight float rows [0, rows) of sy, su, sv (sa) -> packed destination rows [row0, row0 + rows); every byte of those tight rows
// is written once, slots without a sample as zero.  Y': (unsigned)(v * f.up); chroma and alpha: MIN(maxv), MAX(0), truncation.
void launch_yuvp_pack(const float* sy, const float* su, const float* sv, const float* sa, unsigned w, unsigned rows,
                      const YuvPackedRule& f, unsigned char* dst, size_t pitch, unsigned row0, hipStream_t s);

}  // namespace srcnn
