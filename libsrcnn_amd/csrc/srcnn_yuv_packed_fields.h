// srcnn_yuv_packed_fields.h -- the six memory layouts of the packed YUV formats (YuvPackedKind), each stated ONCE: the samples of
// a 16-byte chunk (PkShape), its four dwords <-> field values (decode, encode; luma_field: one luma sample off its one dword), the
// dword access in pieces of the alignment a frame has (load_dword, store_dword; io_of is srcnn_frame_rules.h) and the float ->
// field conversion of the pack side (to_word).  The whole-frame kernels (srcnn_yuv_packed.hip: k_yuvp_unpack, k_yuvp_pack), the
// window kernels behind the packed rect call (srcnn_yuv_packed_window.hip: k_yuvp_window_y, k_yuvp_window_merge) and the kernels
// of the packed rect list call (srcnn_yuv_packed_rect_list.hip) include it, which is why a rect holds the bytes of the frame.
// Everything has internal linkage, as it had inside srcnn_yuv_packed.hip.  Internal, HIP only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_frame_rules.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

// samples of Y, of each chroma plane and of alpha in one 16-byte chunk
template <int K> struct PkShape;
template <> struct PkShape<kPk422x8>  { static constexpr unsigned NY = 8, NC = 4, NA = 0; };
template <> struct PkShape<kPk422x16> { static constexpr unsigned NY = 4, NC = 2, NA = 0; };
template <> struct PkShape<kPk444x8>  { static constexpr unsigned NY = 4, NC = 4, NA = 4; };
template <> struct PkShape<kPk410>    { static constexpr unsigned NY = 4, NC = 4, NA = 4; };
template <> struct PkShape<kPk444x16> { static constexpr unsigned NY = 2, NC = 2, NA = 2; };
template <> struct PkShape<kPkV210>   { static constexpr unsigned NY = 6, NC = 3, NA = 0; };

// (kIoVec / kIoDword / kIoWord / kIoByte and io_of: srcnn_frame_rules.h, which the host-only route code shares)

template <bool SAT>
__device__ __forceinline__ unsigned to_word(float v, float scale, float maxv)
{
    if constexpr (SAT) return (unsigned)saturate(v, maxv);
    else return (unsigned)(v * scale);
}

__device__ __forceinline__ unsigned load_dword(const unsigned char* p, int io)
{
    if (io == kIoByte) return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
    if (io == kIoWord) {
        const unsigned short* ps = reinterpret_cast<const unsigned short*>(p);
        return (unsigned)ps[0] | ((unsigned)ps[1] << 16);
    }
    return *reinterpret_cast<const unsigned*>(p);
}

__device__ __forceinline__ void store_dword(unsigned char* p, unsigned v, int io)
{
    if (io == kIoByte) {
        p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24);
    } else if (io == kIoWord) {
        unsigned short* ps = reinterpret_cast<unsigned short*>(p);
        ps[0] = (unsigned short)v; ps[1] = (unsigned short)(v >> 16);
    } else {
        *reinterpret_cast<unsigned*>(p) = v;
    }
}

// the four dwords of a chunk -> field values (every slot of the chunk, valid or not)
template <int K>
__device__ __forceinline__ void decode(const unsigned q[4], const YuvPackedRule& f, unsigned* y, unsigned* u, unsigned* v, unsigned* a)
{
    if constexpr (K == kPk422x8) {
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            y[2 * j] = (q[j] >> f.sh[0]) & 0xffu; u[j] = (q[j] >> f.sh[1]) & 0xffu;
            y[2 * j + 1] = (q[j] >> f.sh[2]) & 0xffu; v[j] = (q[j] >> f.sh[3]) & 0xffu;
        }
    } else if constexpr (K == kPk422x16) {
#pragma unroll
        for (unsigned j = 0; j < 2; ++j) {
            y[2 * j] = ((q[2 * j] & 0xffffu) >> f.shift) & f.mask; u[j] = ((q[2 * j] >> 16) >> f.shift) & f.mask;
            y[2 * j + 1] = ((q[2 * j + 1] & 0xffffu) >> f.shift) & f.mask; v[j] = ((q[2 * j + 1] >> 16) >> f.shift) & f.mask;
        }
    } else if constexpr (K == kPk444x8) {
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            y[j] = (q[j] >> f.sh[0]) & 0xffu; u[j] = (q[j] >> f.sh[1]) & 0xffu;
            v[j] = (q[j] >> f.sh[2]) & 0xffu; a[j] = (q[j] >> f.sh[3]) & 0xffu;
        }
    } else if constexpr (K == kPk410) {
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            u[j] = q[j] & 0x3ffu; y[j] = (q[j] >> 10) & 0x3ffu; v[j] = (q[j] >> 20) & 0x3ffu; a[j] = q[j] >> 30;
        }
    } else if constexpr (K == kPk444x16) {
#pragma unroll
        for (unsigned j = 0; j < 2; ++j) {
            u[j] = q[2 * j] & 0xffffu; y[j] = q[2 * j] >> 16; v[j] = q[2 * j + 1] & 0xffffu; a[j] = q[2 * j + 1] >> 16;
        }
    } else {                             // v210: Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
        u[0] = q[0] & 0x3ffu; y[0] = (q[0] >> 10) & 0x3ffu; v[0] = (q[0] >> 20) & 0x3ffu;
        y[1] = q[1] & 0x3ffu; u[1] = (q[1] >> 10) & 0x3ffu; y[2] = (q[1] >> 20) & 0x3ffu;
        v[1] = q[2] & 0x3ffu; y[3] = (q[2] >> 10) & 0x3ffu; u[2] = (q[2] >> 20) & 0x3ffu;
        y[4] = q[3] & 0x3ffu; v[2] = (q[3] >> 10) & 0x3ffu; y[5] = (q[3] >> 20) & 0x3ffu;
    }
}

// The luma field of pixel x of a packed row, as decode<K> gives it, from the ONE dword of the row that holds it (in pieces of
// `io`): the other dwords of the pixel's unit are not loaded.
template <int K>
__device__ __forceinline__ unsigned luma_field(const unsigned char* row, size_t x, const YuvPackedRule& f, int io)
{
    if constexpr (K == kPk422x8) {
        return (load_dword(row + 4 * (x / 2), io) >> ((x & 1) ? f.sh[2] : f.sh[0])) & 0xffu;
    } else if constexpr (K == kPk422x16) {
        return ((load_dword(row + 4 * x, io) & 0xffffu) >> f.shift) & f.mask;
    } else if constexpr (K == kPk444x8) {
        return (load_dword(row + 4 * x, io) >> f.sh[0]) & 0xffu;
    } else if constexpr (K == kPk410) {
        return (load_dword(row + 4 * x, io) >> 10) & 0x3ffu;
    } else if constexpr (K == kPk444x16) {
        return load_dword(row + 8 * x, io) >> 16;
    } else {                             // v210: Y0 in dword 0, Y1 Y2 in 1, Y3 in 2, Y4 Y5 in 3
        const unsigned k = (unsigned)(x % 6);
        const unsigned dw = (k + 1) / 2 + (k == 4 ? 1u : 0u);                        // 0 1 1 2 3 3
        const unsigned sh = (k == 0 || k == 3) ? 10u : ((k == 1 || k == 4) ? 0u : 20u);
        return (load_dword(row + 16 * (x / 6) + 4 * dw, io) >> sh) & 0x3ffu;
    }
}

// field values (already inside their fields' ranges; zero where the slot carries no sample) -> the four dwords of a chunk
template <int K>
__device__ __forceinline__ void encode(const unsigned* y, const unsigned* u, const unsigned* v, const unsigned* a, const YuvPackedRule& f, unsigned q[4])
{
    if constexpr (K == kPk422x8) {
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) q[j] = (y[2 * j] << f.sh[0]) | (u[j] << f.sh[1]) | (y[2 * j + 1] << f.sh[2]) | (v[j] << f.sh[3]);
    } else if constexpr (K == kPk422x16) {
#pragma unroll
        for (unsigned j = 0; j < 2; ++j) {
            q[2 * j] = (y[2 * j] << f.shift) | (u[j] << (16 + f.shift));
            q[2 * j + 1] = (y[2 * j + 1] << f.shift) | (v[j] << (16 + f.shift));
        }
    } else if constexpr (K == kPk444x8) {
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) q[j] = (y[j] << f.sh[0]) | (u[j] << f.sh[1]) | (v[j] << f.sh[2]) | (a[j] << f.sh[3]);
    } else if constexpr (K == kPk410) {
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) q[j] = u[j] | (y[j] << 10) | (v[j] << 20) | (a[j] << 30);
    } else if constexpr (K == kPk444x16) {
#pragma unroll
        for (unsigned j = 0; j < 2; ++j) {
            q[2 * j] = u[j] | (y[j] << 16);
            q[2 * j + 1] = v[j] | (a[j] << 16);
        }
    } else {
        q[0] = u[0] | (y[0] << 10) | (v[0] << 20);
        q[1] = y[1] | (u[1] << 10) | (y[2] << 20);
        q[2] = v[1] | (y[3] << 10) | (u[2] << 20);
        q[3] = y[4] | (v[2] << 10) | (y[5] << 20);
    }
}

}  // namespace

}  // namespace srcnn
