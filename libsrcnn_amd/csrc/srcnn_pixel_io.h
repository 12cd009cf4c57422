// srcnn_pixel_io.h -- what the conversion kernels (srcnn_yuv_planes.hip, srcnn_yuv_packed.hip, srcnn_rgb.hip and the window
// kernels) share of memory access: the launch-time alignment test and grid size, the float4-or-scalar access to a piece of a
// tight float row, and the samples of 8-bit / 16-bit words packed in consecutive dwords.  (Their arithmetic is
// srcnn_colour_rules.h.)  Internal, HIP only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace srcnn {

// a NULL pointer is a plane the launch does not have: it never stands in the way of vector accesses
inline bool aligned_to(const void* p, size_t a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// blocks of 256 threads for a grid-stride loop over `total` items, at most `cap` of them
inline dim3 grid_for(size_t total, unsigned cap) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, cap))); }

// N floats at p (N even) as 16-byte or 8-byte stores.  The unpack kernels of srcnn_yuv_planes.hip and srcnn_rgb.hip call it
// for all their planes under ONE branch, with a hand-written tail that goes sample by sample across the planes: that is the
// shape that keeps one dwordx4 store per plane and the instruction count of the kernels.
template <unsigned N>
__device__ __forceinline__ void store_floats_vec(float* p, const float* v)
{
    // (vector types, not the float4 / float2 structs: a struct is stored member by member, and the compiler may move single
    // members out of the branch before it puts the rest together again -- a dwordx3 and a dword instead of a dwordx4)
    typedef float vec4 __attribute__((ext_vector_type(4)));
    typedef float vec2 __attribute__((ext_vector_type(2)));
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (unsigned k = 0; k < N; k += 4) *reinterpret_cast<vec4*>(p + k) = vec4{v[k], v[k + 1], v[k + 2], v[k + 3]};
    } else {
#pragma unroll
        for (unsigned k = 0; k < N; k += 2) *reinterpret_cast<vec2*>(p + k) = vec2{v[k], v[k + 1]};
    }
}

// N floats at p, the first n of them valid: vector accesses for a whole piece where the launch allows them
template <unsigned N>
__device__ __forceinline__ void store_floats(float* p, const float* v, unsigned n, int vec)
{
    if constexpr (N == 0) return;
    if (vec && n == N && N % 2 == 0) {
        if constexpr (N % 2 == 0) store_floats_vec<N>(p, v);
    } else {
#pragma unroll
        for (unsigned k = 0; k < N; ++k)
            if (k < n) p[k] = v[k];
    }
}

template <unsigned N>
__device__ __forceinline__ void load_floats(const float* p, float* v, unsigned n, int vec)
{
    if constexpr (N == 0) return;
    if (vec && n == N && N % 2 == 0) {
        if constexpr (N % 4 == 0) {
#pragma unroll
            for (unsigned k = 0; k < N; k += 4) {
                const float4 x = *reinterpret_cast<const float4*>(p + k);
                v[k] = x.x; v[k + 1] = x.y; v[k + 2] = x.z; v[k + 3] = x.w;
            }
        } else if constexpr (N % 2 == 0) {
#pragma unroll
            for (unsigned k = 0; k < N; k += 2) {
                const float2 x = *reinterpret_cast<const float2*>(p + k);
                v[k] = x.x; v[k + 1] = x.y;
            }
        }
    } else {
#pragma unroll
        for (unsigned k = 0; k < N; ++k) v[k] = k < n ? p[k] : 0.f;
    }
}

// sample j of the samples of BPS bytes packed in consecutive dwords, low address first
template <int BPS>
__device__ __forceinline__ unsigned sample_of(const unsigned* wd, int j)
{
    if constexpr (BPS == 1) return (wd[j >> 2] >> (8 * (j & 3))) & 0xffu;
    else return (wd[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}

// (wd starts as zero; v fits its BPS bytes)
template <int BPS>
__device__ __forceinline__ void put_sample(unsigned* wd, int j, unsigned v)
{
    if constexpr (BPS == 1) wd[j >> 2] |= v << (8 * (j & 3));
    else wd[j >> 1] |= v << (16 * (j & 1));
}

template <int BPS>
__device__ __forceinline__ unsigned load_scalar(const unsigned char* q)
{
    if constexpr (BPS == 1) return *q;
    else return *reinterpret_cast<const unsigned short*>(q);     // 2-byte aligned: the host refuses odd planes
}

template <int BPS>
__device__ __forceinline__ void store_scalar(unsigned char* q, unsigned v)
{
    if constexpr (BPS == 1) *q = (unsigned char)v;
    else *reinterpret_cast<unsigned short*>(q) = (unsigned short)v;
}

}  // namespace srcnn
