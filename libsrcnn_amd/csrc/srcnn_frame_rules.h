// srcnn_frame_rules.h -- what a frame format comes down to for the conversion kernels: plain structs that the host fills in
// (srcnn_frame_args.hpp) and the launchers take (srcnn_yuv.h, srcnn_rgb.h).  No HIP: the host-only sanitizer harness includes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace srcnn {

// ---- planar / semi-planar YUV, 16-bit words of 10 / 12 / 14 / 16 significant bits (include/srcnn_amd_yuv_ex.h) ----
// How a sample of `depth` bits sits in its little-endian 16-bit word, and the exact luma scalings (s = depth - 8).
struct Yuv16Rule {
    unsigned rshift = 0;    // read: (word >> rshift) & mask
    unsigned mask = 0;      // maxv = 2^depth - 1
    unsigned lshift = 0;    // write: value << lshift
    float down = 1.f;       // 2^-s: Y sample -> the Y path's 8-bit scale
    float up = 1.f;         // 2^s:  Yf -> Y'
};

// ---- packed frames: one plane that interleaves Y, U, V (and A) (include/srcnn_amd_yuv_packed.h) ----
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
// tight bytes of a w-pixel packed row (srcnn_yuv_packed_row_bytes): always whole dwords
inline size_t yuv_packed_row_bytes(int kind, unsigned w)
{
    switch (kind) {
    case kPk422x8: return (size_t)4 * ((w + 1) / 2);
    case kPk422x16: return (size_t)8 * ((w + 1) / 2);
    case kPk444x8:
    case kPk410: return (size_t)4 * w;
    case kPk444x16: return (size_t)8 * w;
    default: return (size_t)128 * ((w + 47) / 48);
    }
}
// chroma samples of a w-pixel packed row: ceil(w / 2) for the 4:2:2 kinds, else w
inline unsigned yuv_packed_chroma_cols(int kind, unsigned w)
{
    return kind == kPk422x8 || kind == kPk422x16 || kind == kPkV210 ? (w + 1) / 2 : w;
}
// luma columns per chroma column: 2 for the 4:2:2 kinds, else 1
inline unsigned yuv_packed_chroma_step(int kind) { return kind == kPk422x8 || kind == kPk422x16 || kind == kPkV210 ? 2u : 1u; }
// the unit spans of a packed row are made of, in pixels and in bytes (srcnn_yuv_packed_span_bytes): a pixel pair of the 4:2:2
// kinds, a pixel of the 4:4:4 kinds, a v210 group of 6
inline unsigned yuv_packed_unit(int kind) { return kind == kPkV210 ? 6u : yuv_packed_chroma_step(kind); }
inline unsigned yuv_packed_unit_bytes(int kind)
{
    switch (kind) {
    case kPk422x8: case kPk444x8: case kPk410: return 4;
    case kPk422x16: case kPk444x16: return 8;
    default: return 16;
    }
}
// byte offset and byte length of pixels [x, x + n) of a `width`-pixel row: x a multiple of the unit, n one or x + n == width,
// where the length runs to the end of the tight row (the empty slots of the last unit and v210's padding groups included)
inline void yuv_packed_span(int kind, unsigned width, unsigned x, unsigned n, size_t& offset, size_t& bytes)
{
    const unsigned unit = yuv_packed_unit(kind);
    const size_t ub = yuv_packed_unit_bytes(kind);
    offset = (size_t)(x / unit) * ub;
    const size_t end = x + n >= width ? yuv_packed_row_bytes(kind, width) : (size_t)((x + n) / unit) * ub;
    bytes = end - offset;
}
// the chroma tile width of k_yuvp_window_merge: 64, or 60 (20 groups of 3) for v210
inline unsigned yuv_packed_tile_cols(int kind) { return kind == kPkV210 ? 60u : 64u; }
// bytes [blo, bhi) of a row of the w-pixel frame that hold luma columns [lx, hx) widened outward to the unit and cut at w
inline void yuv_packed_unit_span(int kind, unsigned w, unsigned lx, unsigned hx, unsigned& blo, unsigned& bhi)
{
    const unsigned unit = yuv_packed_unit(kind);
    lx -= lx % unit;
    hx = (hx + unit - 1) / unit * unit;
    if (hx > w) hx = w;
    size_t off = 0, n = 0;
    yuv_packed_span(kind, w, lx, hx - lx, off, n);
    blo = (unsigned)off;
    bhi = (unsigned)(off + n);
}
// how the packed side of a launch is addressed: 16-byte vectors, or pieces of 4, 2 or 1 bytes -- by what base and pitch share
enum { kIoVec = 0, kIoDword = 4, kIoWord = 2, kIoByte = 1 };
inline int io_of(const void* base, size_t pitch)
{
    const uintptr_t bits = reinterpret_cast<uintptr_t>(base) | (uintptr_t)pitch;
    return bits % 16 == 0 ? kIoVec : bits % 4 == 0 ? kIoDword : bits % 2 == 0 ? kIoWord : kIoByte;
}

// ---- RGB(A) images (include/srcnn_amd_rgb.h): what a srcnn_rgb_format comes down to (s = depth - 8) ----
struct RgbRule {
    bool planar = false;    // one plane per channel instead of one plane of interleaved pixels
    bool bgr = false;       // the first and the third channel change places
    int ch = 3;             // channels: 3, or 4 with alpha last
    unsigned bps = 1;       // bytes per sample: 1 (depth 8) or 2
    unsigned mask = 0xffu;  // maxv = 2^depth - 1
    float down = 1.f;       // 2^-s: sample -> the 8-bit scale the colour arithmetic works on
    float up = 1.f;         // 2^s:  clamped result -> sample
};

}  // namespace srcnn
