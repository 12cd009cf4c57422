// srcnn_yuv16.hip -- the 16-bit-word conversions around the SRCNN path for YUV frames of 10 / 12 / 14 / 16 significant bits
// (include/srcnn_amd_yuv_ex.h).  One little-endian 16-bit word per sample, the value in its low or in its high bits.
//
//   k_yuv16_unpack   pitched u16 plane (or interleaved UV plane) -> tight float32 plane(s)
//                    value = (word >> rshift) & mask;   float = (float)value * scale     (scale = 2^-s for Y, 1 for chroma:
//                    both exact in fp32)
//   k_yuv16_pack     tight float32 rows -> pitched u16 plane (UV: U, V interleaved)
//                    Y':     (unsigned) (v * scale)                 scale = 2^s; layer 3 already clamps v to [0, 255]
//                    U', V': MIN(maxv), MAX(0), truncation           the reference's macro forms on the native scale
//                    word = value << lshift
//
// rshift, mask, lshift, maxv and scale are kernel arguments: every depth and both alignments run the same few instances.
// Both kernels are memory-bound and move 8 samples per thread: one 16-byte load or store of words (two for a UV plane)
// against two (four) float4, where base and pitch are aligned for it (decided once per launch); a row's last partial chunk
// and misaligned planes take the scalar forms.  Grid-stride over rows x chunks.  The host side is srcnn_capi.cpp
// (srcnn_yuv_upscale_dev); the 8-bit forms are srcnn_yuv.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "srcnn_yuv.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr unsigned kChunk16 = 8;         // samples per thread and plane

template <bool SAT>
__device__ __forceinline__ unsigned to_word(float v, float scale, float maxv, unsigned lshift)
{
    if constexpr (SAT) {                 // MIN(maxv, v) then MAX(0.f, .) then truncating cast, in the reference's macro forms
        v = (maxv < v) ? maxv : v;
        v = (0.f > v) ? 0.f : v;
        return (unsigned)v << lshift;
    } else {
        return (unsigned)(v * scale) << lshift;
    }
}

// the two 16-bit words of a dword, low address first
__device__ __forceinline__ void split2(unsigned q, unsigned rshift, unsigned mask, float scale, float& lo, float& hi)
{
    lo = (float)(((q & 0xffffu) >> rshift) & mask) * scale;
    hi = (float)(((q >> 16) >> rshift) & mask) * scale;
}

// src_vec: every row start is 16-byte aligned; dst_vec: every float row start is 16-byte aligned.  UV: `w` (U, V) word
// pairs per row -> d0 (U), d1 (V).
template <bool UV>
__global__ __launch_bounds__(256) void k_yuv16_unpack(const unsigned char* __restrict__ src, size_t pitch, unsigned w,
                                                      unsigned rows, float* __restrict__ d0, float* __restrict__ d1,
                                                      unsigned rshift, unsigned mask, float scale, int src_vec, int dst_vec)
{
    const unsigned cpr = (w + kChunk16 - 1) / kChunk16;
    const unsigned total = cpr * rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * kChunk16;
        const unsigned n = min(kChunk16, w - c);
        const unsigned char* p = src + (size_t)r * pitch + (size_t)(UV ? 4 : 2) * c;
        const size_t o = (size_t)r * w + c;
        float a[kChunk16], b[kChunk16];
        if (n == kChunk16 && src_vec) {
            if constexpr (UV) {
                const uint4 q0 = *reinterpret_cast<const uint4*>(p);
                const uint4 q1 = *reinterpret_cast<const uint4*>(p + 16);
                split2(q0.x, rshift, mask, scale, a[0], b[0]); split2(q0.y, rshift, mask, scale, a[1], b[1]);
                split2(q0.z, rshift, mask, scale, a[2], b[2]); split2(q0.w, rshift, mask, scale, a[3], b[3]);
                split2(q1.x, rshift, mask, scale, a[4], b[4]); split2(q1.y, rshift, mask, scale, a[5], b[5]);
                split2(q1.z, rshift, mask, scale, a[6], b[6]); split2(q1.w, rshift, mask, scale, a[7], b[7]);
            } else {
                const uint4 q = *reinterpret_cast<const uint4*>(p);
                split2(q.x, rshift, mask, scale, a[0], a[1]); split2(q.y, rshift, mask, scale, a[2], a[3]);
                split2(q.z, rshift, mask, scale, a[4], a[5]); split2(q.w, rshift, mask, scale, a[6], a[7]);
            }
        } else {
            const unsigned short* ps = reinterpret_cast<const unsigned short*>(p);   // 2-byte aligned: the host refuses odd planes
#pragma unroll
            for (unsigned k = 0; k < kChunk16; ++k) {
                if (k < n) {
                    if constexpr (UV) {
                        a[k] = (float)(((unsigned)ps[2 * k] >> rshift) & mask) * scale;
                        b[k] = (float)(((unsigned)ps[2 * k + 1] >> rshift) & mask) * scale;
                    } else {
                        a[k] = (float)(((unsigned)ps[k] >> rshift) & mask) * scale;
                    }
                }
            }
        }
        if (n == kChunk16 && dst_vec) {
            *reinterpret_cast<float4*>(d0 + o) = make_float4(a[0], a[1], a[2], a[3]);
            *reinterpret_cast<float4*>(d0 + o + 4) = make_float4(a[4], a[5], a[6], a[7]);
            if constexpr (UV) {
                *reinterpret_cast<float4*>(d1 + o) = make_float4(b[0], b[1], b[2], b[3]);
                *reinterpret_cast<float4*>(d1 + o + 4) = make_float4(b[4], b[5], b[6], b[7]);
            }
        } else {
#pragma unroll
            for (unsigned k = 0; k < kChunk16; ++k) {
                if (k < n) {
                    d0[o + k] = a[k];
                    if constexpr (UV) d1[o + k] = b[k];
                }
            }
        }
    }
}

// src_vec: every float row start is 16-byte aligned; dst_vec: every destination row start is 16-byte aligned.  Source row r
// goes to destination row row0 + r.
template <bool UV, bool SAT>
__global__ __launch_bounds__(256) void k_yuv16_pack(const float* __restrict__ s0, const float* __restrict__ s1, unsigned w,
                                                    unsigned rows, unsigned char* __restrict__ dst, size_t pitch, unsigned row0,
                                                    float scale, float maxv, unsigned lshift, int src_vec, int dst_vec)
{
    const unsigned cpr = (w + kChunk16 - 1) / kChunk16;
    const unsigned total = cpr * rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * kChunk16;
        const unsigned n = min(kChunk16, w - c);
        const size_t o = (size_t)r * w + c;
        unsigned char* q = dst + (size_t)(row0 + r) * pitch + (size_t)(UV ? 4 : 2) * c;
        float a[kChunk16], b[kChunk16];
        if (n == kChunk16 && src_vec) {
            const float4 x0 = *reinterpret_cast<const float4*>(s0 + o);
            const float4 x1 = *reinterpret_cast<const float4*>(s0 + o + 4);
            a[0] = x0.x; a[1] = x0.y; a[2] = x0.z; a[3] = x0.w; a[4] = x1.x; a[5] = x1.y; a[6] = x1.z; a[7] = x1.w;
            if constexpr (UV) {
                const float4 y0 = *reinterpret_cast<const float4*>(s1 + o);
                const float4 y1 = *reinterpret_cast<const float4*>(s1 + o + 4);
                b[0] = y0.x; b[1] = y0.y; b[2] = y0.z; b[3] = y0.w; b[4] = y1.x; b[5] = y1.y; b[6] = y1.z; b[7] = y1.w;
            }
        } else {
#pragma unroll
            for (unsigned k = 0; k < kChunk16; ++k) {
                a[k] = k < n ? s0[o + k] : 0.f;
                if constexpr (UV) b[k] = k < n ? s1[o + k] : 0.f;
            }
        }
        unsigned wa[kChunk16], wb[kChunk16];
#pragma unroll
        for (unsigned k = 0; k < kChunk16; ++k) {
            wa[k] = to_word<SAT>(a[k], scale, maxv, lshift);
            if constexpr (UV) wb[k] = to_word<SAT>(b[k], scale, maxv, lshift);
        }
        if (n == kChunk16 && dst_vec) {
            if constexpr (UV) {
                *reinterpret_cast<uint4*>(q) = make_uint4(wa[0] | (wb[0] << 16), wa[1] | (wb[1] << 16), wa[2] | (wb[2] << 16), wa[3] | (wb[3] << 16));
                *reinterpret_cast<uint4*>(q + 16) = make_uint4(wa[4] | (wb[4] << 16), wa[5] | (wb[5] << 16), wa[6] | (wb[6] << 16), wa[7] | (wb[7] << 16));
            } else {
                *reinterpret_cast<uint4*>(q) = make_uint4(wa[0] | (wa[1] << 16), wa[2] | (wa[3] << 16), wa[4] | (wa[5] << 16), wa[6] | (wa[7] << 16));
            }
        } else {
            unsigned short* qs = reinterpret_cast<unsigned short*>(q);               // 2-byte aligned, as in the unpack
#pragma unroll
            for (unsigned k = 0; k < kChunk16; ++k) {
                if (k < n) {
                    if constexpr (UV) { qs[2 * k] = (unsigned short)wa[k]; qs[2 * k + 1] = (unsigned short)wb[k]; }
                    else qs[k] = (unsigned short)wa[k];
                }
            }
        }
    }
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

dim3 grid_for(unsigned w, unsigned rows)
{
    const size_t total = (size_t)((w + kChunk16 - 1) / kChunk16) * rows;
    return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, 4096)));
}

}  // namespace

void launch_yuv16_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, bool uv, const Yuv16Rule& f,
                         bool luma, float* d0, float* d1, hipStream_t s)
{
    const int src_vec = aligned_to(src, 16) && pitch % 16 == 0;
    const int dst_vec = w % 4 == 0 && aligned_to(d0, 16) && (!uv || aligned_to(d1, 16));
    const float scale = luma ? f.down : 1.f;
    if (uv) hipLaunchKernelGGL(k_yuv16_unpack<true>, grid_for(w, rows), dim3(256), 0, s, src, pitch, w, rows, d0, d1, f.rshift, f.mask, scale, src_vec, dst_vec);
    else hipLaunchKernelGGL(k_yuv16_unpack<false>, grid_for(w, rows), dim3(256), 0, s, src, pitch, w, rows, d0, d1, f.rshift, f.mask, scale, src_vec, dst_vec);
}

void launch_yuv16_pack(const float* s0, const float* s1, unsigned w, unsigned rows, bool sat, const Yuv16Rule& f,
                       unsigned char* dst, size_t pitch, unsigned row0, hipStream_t s)
{
    const bool uv = s1 != nullptr;       // an interleaved plane is a chroma plane: always saturated
    const int src_vec = w % 4 == 0 && aligned_to(s0, 16) && (!uv || aligned_to(s1, 16));
    const int dst_vec = aligned_to(dst, 16) && pitch % 16 == 0;
    const dim3 g = grid_for(w, rows);
    const float maxv = (float)f.mask;
    if (uv) hipLaunchKernelGGL((k_yuv16_pack<true, true>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, f.up, maxv, f.lshift, src_vec, dst_vec);
    else if (sat) hipLaunchKernelGGL((k_yuv16_pack<false, true>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, f.up, maxv, f.lshift, src_vec, dst_vec);
    else hipLaunchKernelGGL((k_yuv16_pack<false, false>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, f.up, maxv, f.lshift, src_vec, dst_vec);
}

}  // namespace srcnn
