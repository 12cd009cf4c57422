// srcnn_yuv.hip -- the 8-bit conversions around the SRCNN path for YUV 4:2:0 frames (include/srcnn_amd_yuv.h).
//
//   k_yuv_unpack   pitched u8 plane (or interleaved NV12 UV plane) -> tight float32 plane(s)   (float)Y, (float)U, (float)V
//   k_yuv_pack     tight float32 rows -> pitched u8 plane (NV12: U, V interleaved)
//                  Y':     (unsigned char) v            as conv_opt in k_ycc_merge (src/libsrcnn.cpp:889-905)
//                  U', V': MIN(255), MAX(0), truncation  as to_u8_sat in srcnn_kernels.hip
//
// Both are memory-bound and move 4 samples per thread: a dword (I420) or two dwords (NV12) of bytes, a float4 per float
// plane, where base and pitch are aligned for it (decided once per launch); a row's last partial chunk and misaligned
// planes take the byte / scalar forms.  Grid-stride over rows x chunks.  The host side is srcnn_capi.cpp
// (srcnn_yuv420_upscale_dev).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "srcnn_yuv.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

__device__ __forceinline__ unsigned char yuv_u8_sat(float v)
{   // MIN(255.f, v) then MAX(0.f, .) then truncating cast, in the reference's macro forms (the same as to_u8_sat)
    v = (255.f < v) ? 255.f : v;
    v = (0.f > v) ? 0.f : v;
    return (unsigned char)v;
}

template <bool SAT>
__device__ __forceinline__ unsigned to_u8(float v)
{
    if constexpr (SAT) return yuv_u8_sat(v);
    else return (unsigned char)v;
}

constexpr unsigned kChunk = 4;           // samples per thread and plane

// src_vec: every row start is 4-byte (I420) / 8-byte (NV12) aligned; dst_vec: every float row start is 16-byte aligned
template <bool NV12>
__global__ __launch_bounds__(256) void k_yuv_unpack(const unsigned char* __restrict__ src, size_t pitch, unsigned w,
                                                    unsigned rows, float* __restrict__ d0, float* __restrict__ d1, int src_vec,
                                                    int dst_vec)
{
    const unsigned cpr = (w + kChunk - 1) / kChunk;
    const unsigned total = cpr * rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * kChunk;
        const unsigned n = min(kChunk, w - c);
        const unsigned char* p = src + (size_t)r * pitch + (NV12 ? 2 * c : c);
        const size_t o = (size_t)r * w + c;
        float a[kChunk], b[kChunk];
        if (n == kChunk && src_vec) {
            if constexpr (NV12) {
                const uint2 q = *reinterpret_cast<const uint2*>(p);
                a[0] = (float)(q.x & 0xffu); b[0] = (float)((q.x >> 8) & 0xffu);
                a[1] = (float)((q.x >> 16) & 0xffu); b[1] = (float)(q.x >> 24);
                a[2] = (float)(q.y & 0xffu); b[2] = (float)((q.y >> 8) & 0xffu);
                a[3] = (float)((q.y >> 16) & 0xffu); b[3] = (float)(q.y >> 24);
            } else {
                const unsigned q = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
                for (unsigned k = 0; k < kChunk; ++k) a[k] = (float)((q >> (8 * k)) & 0xffu);
            }
        } else {
#pragma unroll
            for (unsigned k = 0; k < kChunk; ++k) {
                if (k < n) {
                    if constexpr (NV12) { a[k] = (float)p[2 * k]; b[k] = (float)p[2 * k + 1]; }
                    else a[k] = (float)p[k];
                }
            }
        }
        if (n == kChunk && dst_vec) {
            *reinterpret_cast<float4*>(d0 + o) = make_float4(a[0], a[1], a[2], a[3]);
            if constexpr (NV12) *reinterpret_cast<float4*>(d1 + o) = make_float4(b[0], b[1], b[2], b[3]);
        } else {
#pragma unroll
            for (unsigned k = 0; k < kChunk; ++k) {
                if (k < n) {
                    d0[o + k] = a[k];
                    if constexpr (NV12) d1[o + k] = b[k];
                }
            }
        }
    }
}

// src_vec: every float row start is 16-byte aligned; dst_vec: every destination row start is 4-byte (I420) / 8-byte (NV12)
// aligned.  Source row r goes to destination row row0 + r.
template <bool NV12, bool SAT>
__global__ __launch_bounds__(256) void k_yuv_pack(const float* __restrict__ s0, const float* __restrict__ s1, unsigned w,
                                                  unsigned rows, unsigned char* __restrict__ dst, size_t pitch, unsigned row0,
                                                  int src_vec, int dst_vec)
{
    const unsigned cpr = (w + kChunk - 1) / kChunk;
    const unsigned total = cpr * rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * kChunk;
        const unsigned n = min(kChunk, w - c);
        const size_t o = (size_t)r * w + c;
        unsigned char* q = dst + (size_t)(row0 + r) * pitch + (NV12 ? 2 * c : c);
        float a[kChunk], b[kChunk];
        if (n == kChunk && src_vec) {
            const float4 x = *reinterpret_cast<const float4*>(s0 + o);
            a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w;
            if constexpr (NV12) {
                const float4 y = *reinterpret_cast<const float4*>(s1 + o);
                b[0] = y.x; b[1] = y.y; b[2] = y.z; b[3] = y.w;
            }
        } else {
#pragma unroll
            for (unsigned k = 0; k < kChunk; ++k) {
                a[k] = k < n ? s0[o + k] : 0.f;
                if constexpr (NV12) b[k] = k < n ? s1[o + k] : 0.f;
            }
        }
        if (n == kChunk && dst_vec) {
            if constexpr (NV12) {
                uint2 v;
                v.x = to_u8<SAT>(a[0]) | (to_u8<SAT>(b[0]) << 8) | (to_u8<SAT>(a[1]) << 16) | (to_u8<SAT>(b[1]) << 24);
                v.y = to_u8<SAT>(a[2]) | (to_u8<SAT>(b[2]) << 8) | (to_u8<SAT>(a[3]) << 16) | (to_u8<SAT>(b[3]) << 24);
                *reinterpret_cast<uint2*>(q) = v;
            } else {
                *reinterpret_cast<unsigned*>(q) =
                    to_u8<SAT>(a[0]) | (to_u8<SAT>(a[1]) << 8) | (to_u8<SAT>(a[2]) << 16) | (to_u8<SAT>(a[3]) << 24);
            }
        } else {
#pragma unroll
            for (unsigned k = 0; k < kChunk; ++k) {
                if (k < n) {
                    if constexpr (NV12) { q[2 * k] = (unsigned char)to_u8<SAT>(a[k]); q[2 * k + 1] = (unsigned char)to_u8<SAT>(b[k]); }
                    else q[k] = (unsigned char)to_u8<SAT>(a[k]);
                }
            }
        }
    }
}

inline bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

dim3 grid_for(unsigned w, unsigned rows)
{
    const size_t total = (size_t)((w + kChunk - 1) / kChunk) * rows;
    return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, 4096)));
}

}  // namespace

void launch_yuv_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, bool nv12, float* d0, float* d1,
                       hipStream_t s)
{
    const size_t sa = nv12 ? 8 : 4;
    const int src_vec = aligned_to(src, sa) && pitch % sa == 0;
    const int dst_vec = w % 4 == 0 && aligned_to(d0, 16) && (!nv12 || aligned_to(d1, 16));
    if (nv12) hipLaunchKernelGGL(k_yuv_unpack<true>, grid_for(w, rows), dim3(256), 0, s, src, pitch, w, rows, d0, d1, src_vec, dst_vec);
    else hipLaunchKernelGGL(k_yuv_unpack<false>, grid_for(w, rows), dim3(256), 0, s, src, pitch, w, rows, d0, d1, src_vec, dst_vec);
}

void launch_yuv_pack(const float* s0, const float* s1, unsigned w, unsigned rows, bool sat, unsigned char* dst, size_t pitch,
                     unsigned row0, hipStream_t s)
{
    const bool nv12 = s1 != nullptr;
    const size_t da = nv12 ? 8 : 4;
    const int src_vec = w % 4 == 0 && aligned_to(s0, 16) && (!nv12 || aligned_to(s1, 16));
    const int dst_vec = aligned_to(dst, da) && pitch % da == 0;
    const dim3 g = grid_for(w, rows);
    if (nv12 && sat) hipLaunchKernelGGL((k_yuv_pack<true, true>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, src_vec, dst_vec);
    else if (nv12) hipLaunchKernelGGL((k_yuv_pack<true, false>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, src_vec, dst_vec);
    else if (sat) hipLaunchKernelGGL((k_yuv_pack<false, true>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, src_vec, dst_vec);
    else hipLaunchKernelGGL((k_yuv_pack<false, false>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, src_vec, dst_vec);
}

}  // namespace srcnn
