// srcnn_yuv_planes.hip -- the conversions around the SRCNN path for planar and semi-planar YUV frames
// (include/srcnn_amd_yuv.h: 8-bit 4:2:0; include/srcnn_amd_yuv_ex.h: every depth and chroma format).  A sample is a byte
// (BPS == 1) or a little-endian 16-bit word with 10 / 12 / 14 / 16 significant bits in its low or its high end (BPS == 2).
//
//   k_plane_unpack<BPS, UV>      pitched plane (UV: interleaved U, V samples) -> tight float32 plane(s)
//                                BPS 1: (float)byte
//                                BPS 2: value = (word >> rshift) & mask;  float = (float)value * scale   (scale = 2^-s for Y,
//                                       1 for chroma: both exact in fp32)
//   k_plane_pack<BPS, UV, SAT>   tight float32 rows -> pitched plane (UV: U, V interleaved)
//                                Y' (!SAT):     (unsigned char) v, or (unsigned)(v * 2^s) << lshift: layer 3 already clamps
//                                               v to [0, 255], like conv_opt in k_ycc_merge (src/libsrcnn.cpp:889-905)
//                                U', V' (SAT):  MIN(maxv), MAX(0), truncation on the native scale, << lshift: the reference's
//                                               macro forms, as to_u8_sat in srcnn_kernels.hip
// The saturation and the word read are srcnn_colour_rules.h, shared with the window kernel of srcnn_yuv_window.hip.
//
// rshift, mask, lshift, maxv and scale are kernel arguments, so every depth and both alignments run the same few 16-bit
// instances; the 8-bit instances compile them out.  Both kernels are memory-bound and move 4 * BPS samples per thread and
// plane: a dword of bytes or 16 bytes of words (twice that for a UV plane) against one or two float4 per float plane, where
// base and pitch are aligned for it (decided once per launch); a row's last partial chunk and misaligned planes take the
// scalar forms.  Grid-stride over rows x chunks.  The host side is srcnn_frames.cpp (yuv_frame).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_yuv.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

template <int BPS, bool SAT>
__device__ __forceinline__ unsigned to_sample(float v, float scale, float maxv, unsigned lshift)
{
    if constexpr (SAT) return to_saturated_sample<BPS>(v, maxv, lshift);
    else if constexpr (BPS == 1) return (unsigned char)v;
    else return (unsigned)(v * scale) << lshift;
}

// ND consecutive dwords as the widest accesses they allow: a dword, a uint2 or uint4s
template <unsigned ND>
__device__ __forceinline__ void load_dwords(const unsigned char* p, unsigned* q)
{
    if constexpr (ND == 1) q[0] = *reinterpret_cast<const unsigned*>(p);
    else if constexpr (ND == 2) {
        const uint2 x = *reinterpret_cast<const uint2*>(p);
        q[0] = x.x; q[1] = x.y;
    } else {
#pragma unroll
        for (unsigned k = 0; k < ND; k += 4) {
            const uint4 x = *reinterpret_cast<const uint4*>(p + 4 * k);
            q[k] = x.x; q[k + 1] = x.y; q[k + 2] = x.z; q[k + 3] = x.w;
        }
    }
}

template <unsigned ND>
__device__ __forceinline__ void store_dwords(unsigned char* p, const unsigned* q)
{
    if constexpr (ND == 1) *reinterpret_cast<unsigned*>(p) = q[0];
    else if constexpr (ND == 2) *reinterpret_cast<uint2*>(p) = make_uint2(q[0], q[1]);
    else {
#pragma unroll
        for (unsigned k = 0; k < ND; k += 4) *reinterpret_cast<uint4*>(p + 4 * k) = make_uint4(q[k], q[k + 1], q[k + 2], q[k + 3]);
    }
}

// src_vec: every row start is aligned for the chunk's bytes (4, UV 8 at BPS 1; 16 at BPS 2); dst_vec: every float row start is
// 16-byte aligned.  UV: `w` (U, V) sample pairs per row -> d0 (U), d1 (V).
template <int BPS, bool UV>
__global__ __launch_bounds__(256) void k_plane_unpack(const unsigned char* __restrict__ src, size_t pitch, unsigned w,
                                                      unsigned rows, float* __restrict__ d0, float* __restrict__ d1,
                                                      unsigned rshift, unsigned mask, float scale, int src_vec, int dst_vec)
{
    constexpr unsigned N = 4 * BPS;                       // samples per thread and plane
    constexpr unsigned ND = N * BPS * (UV ? 2 : 1) / 4;   // dwords of a whole chunk
    const unsigned cpr = (w + N - 1) / N;
    const unsigned total = cpr * rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * N;
        const unsigned n = min(N, w - c);
        const unsigned char* p = src + (size_t)r * pitch + (size_t)(UV ? 2 : 1) * BPS * c;
        unsigned a[N] = {}, b[N] = {};
        if (n == N && src_vec) {
            unsigned q[ND];
            load_dwords<ND>(p, q);
#pragma unroll
            for (unsigned k = 0; k < N; ++k) {
                if constexpr (UV) { a[k] = sample_of<BPS>(q, 2 * k); b[k] = sample_of<BPS>(q, 2 * k + 1); }
                else a[k] = sample_of<BPS>(q, k);
            }
        } else {
#pragma unroll
            for (unsigned k = 0; k < N; ++k) {
                if (k < n) {
                    if constexpr (UV) { a[k] = load_scalar<BPS>(p + 2 * k * BPS); b[k] = load_scalar<BPS>(p + (2 * k + 1) * BPS); }
                    else a[k] = load_scalar<BPS>(p + k * BPS);
                }
            }
        }
        float fa[N], fb[N];
#pragma unroll
        for (unsigned k = 0; k < N; ++k) {
            if constexpr (BPS == 1) { fa[k] = (float)a[k]; fb[k] = (float)b[k]; }
            else { fa[k] = (float)word_value(a[k], rshift, mask) * scale; fb[k] = (float)word_value(b[k], rshift, mask) * scale; }
        }
        const size_t o = (size_t)r * w + c;
        if (n == N && dst_vec) {
            store_floats_vec<N>(d0 + o, fa);
            if constexpr (UV) store_floats_vec<N>(d1 + o, fb);
        } else {
#pragma unroll
            for (unsigned k = 0; k < N; ++k) {
                if (k < n) {
                    d0[o + k] = fa[k];
                    if constexpr (UV) d1[o + k] = fb[k];
                }
            }
        }
    }
}

// src_vec: every float row start is 16-byte aligned; dst_vec: every destination row start is aligned for the chunk's bytes, as
// in the unpack.  Source row r goes to destination row row0 + r.
template <int BPS, bool UV, bool SAT>
__global__ __launch_bounds__(256) void k_plane_pack(const float* __restrict__ s0, const float* __restrict__ s1, unsigned w,
                                                    unsigned rows, unsigned char* __restrict__ dst, size_t pitch, unsigned row0,
                                                    float scale, float maxv, unsigned lshift, int src_vec, int dst_vec)
{
    constexpr unsigned N = 4 * BPS;
    constexpr unsigned ND = N * BPS * (UV ? 2 : 1) / 4;
    const unsigned cpr = (w + N - 1) / N;
    const unsigned total = cpr * rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * N;
        const unsigned n = min(N, w - c);
        const size_t o = (size_t)r * w + c;
        unsigned char* p = dst + (size_t)(row0 + r) * pitch + (size_t)(UV ? 2 : 1) * BPS * c;
        float fa[N], fb[N];
        load_floats<N>(s0 + o, fa, n, src_vec);
        if constexpr (UV) load_floats<N>(s1 + o, fb, n, src_vec);
        unsigned a[N], b[N];
#pragma unroll
        for (unsigned k = 0; k < N; ++k) {
            a[k] = to_sample<BPS, SAT>(fa[k], scale, maxv, lshift);
            b[k] = 0;
            if constexpr (UV) b[k] = to_sample<BPS, SAT>(fb[k], scale, maxv, lshift);
        }
        if (n == N && dst_vec) {
            unsigned q[ND] = {};
#pragma unroll
            for (unsigned k = 0; k < N; ++k) {
                if constexpr (UV) { put_sample<BPS>(q, 2 * k, a[k]); put_sample<BPS>(q, 2 * k + 1, b[k]); }
                else put_sample<BPS>(q, k, a[k]);
            }
            store_dwords<ND>(p, q);
        } else {
#pragma unroll
            for (unsigned k = 0; k < N; ++k) {
                if (k < n) {
                    if constexpr (UV) { store_scalar<BPS>(p + 2 * k * BPS, a[k]); store_scalar<BPS>(p + (2 * k + 1) * BPS, b[k]); }
                    else store_scalar<BPS>(p + k * BPS, a[k]);
                }
            }
        }
    }
}

constexpr unsigned kGridCap = 4096;

template <int BPS>
void plane_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, bool uv, unsigned rshift, unsigned mask,
                  float scale, float* d0, float* d1, hipStream_t s)
{
    const size_t sa = BPS == 2 ? 16 : uv ? 8 : 4;
    const int src_vec = aligned_to(src, sa) && pitch % sa == 0;
    const int dst_vec = w % 4 == 0 && aligned_to(d0, 16) && aligned_to(d1, 16);
    const dim3 g = grid_for((size_t)((w + 4 * BPS - 1) / (4 * BPS)) * rows, kGridCap);
    if (uv) hipLaunchKernelGGL((k_plane_unpack<BPS, true>), g, dim3(256), 0, s, src, pitch, w, rows, d0, d1, rshift, mask, scale, src_vec, dst_vec);
    else hipLaunchKernelGGL((k_plane_unpack<BPS, false>), g, dim3(256), 0, s, src, pitch, w, rows, d0, d1, rshift, mask, scale, src_vec, dst_vec);
}

template <int BPS>
void plane_pack(const float* s0, const float* s1, unsigned w, unsigned rows, bool sat, float scale, float maxv, unsigned lshift,
                unsigned char* dst, size_t pitch, unsigned row0, hipStream_t s)
{
    const bool uv = s1 != nullptr;       // an interleaved plane is a chroma plane: always saturated
    const size_t da = BPS == 2 ? 16 : uv ? 8 : 4;
    const int src_vec = w % 4 == 0 && aligned_to(s0, 16) && aligned_to(s1, 16);
    const int dst_vec = aligned_to(dst, da) && pitch % da == 0;
    const dim3 g = grid_for((size_t)((w + 4 * BPS - 1) / (4 * BPS)) * rows, kGridCap);
    if (uv) hipLaunchKernelGGL((k_plane_pack<BPS, true, true>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, scale, maxv, lshift, src_vec, dst_vec);
    else if (sat) hipLaunchKernelGGL((k_plane_pack<BPS, false, true>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, scale, maxv, lshift, src_vec, dst_vec);
    else hipLaunchKernelGGL((k_plane_pack<BPS, false, false>), g, dim3(256), 0, s, s0, s1, w, rows, dst, pitch, row0, scale, maxv, lshift, src_vec, dst_vec);
}

}  // namespace

void launch_plane_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, bool uv, const Yuv16Rule* f, bool luma,
                         float* d0, float* d1, hipStream_t s)
{
    if (f) plane_unpack<2>(src, pitch, w, rows, uv, f->rshift, f->mask, luma ? f->down : 1.f, d0, d1, s);
    else plane_unpack<1>(src, pitch, w, rows, uv, 0, 0xffu, 1.f, d0, d1, s);
}

void launch_plane_pack(const float* s0, const float* s1, unsigned w, unsigned rows, bool sat, const Yuv16Rule* f,
                       unsigned char* dst, size_t pitch, unsigned row0, hipStream_t s)
{
    if (f) plane_pack<2>(s0, s1, w, rows, sat, f->up, (float)f->mask, f->lshift, dst, pitch, row0, s);
    else plane_pack<1>(s0, s1, w, rows, sat, 1.f, 255.f, 0, dst, pitch, row0, s);
}

}  // namespace srcnn
