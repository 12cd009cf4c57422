// srcnn_colour_rules.h -- the bit-exact pixel rules of the colour shells, each stated once: the reference's saturation, the
// sample codes built on it, the read of a 16-bit word, and the colour split and merge of src/libsrcnn.cpp.  The whole-frame
// kernels (srcnn_rgb.hip, srcnn_yuv_planes.hip, srcnn_yuv_packed.hip) and the window kernels behind the rect calls
// (srcnn_rgb_window.hip, srcnn_yuv_window.hip, srcnn_yuv_packed_window.hip) call the same functions, which is why a rect holds the bytes of the frame.
// (srcnn_kernels.hip keeps its own statements of the split and merge: its text is fingerprinted, see build.py.)
// Every product and every sum is rounded on its own: no contraction, and the expressions are the reference's, token for
// token.  Internal, HIP only.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace srcnn {

// MIN(maxv, v) then MAX(0.f, .) in the reference's macro forms
__device__ __forceinline__ float saturate(float v, float maxv)
{
    v = (maxv < v) ? maxv : v;
    v = (0.f > v) ? 0.f : v;
    return v;
}

// an RGB(A) sample: saturation to [0, 255], the exact scaling to the format's depth, the truncating cast
__device__ __forceinline__ unsigned to_code(float v, float up) { return (unsigned)(saturate(v, 255.f) * up); }

// a chroma sample of a YUV plane, on the native scale: saturation, the truncating cast, the word's alignment.  8-bit samples
// saturate to the literal 255, so their instances compile maxv and lshift out.
template <int BPS>
__device__ __forceinline__ unsigned to_saturated_sample(float v, float maxv, unsigned lshift)
{
    if constexpr (BPS == 1) return (unsigned char)saturate(v, 255.f);
    else return (unsigned)saturate(v, maxv) << lshift;
}

// the value of a 16-bit word with its significant bits in the low or the high end
__device__ __forceinline__ unsigned word_value(unsigned word, unsigned rshift, unsigned mask) { return (word >> rshift) & mask; }

// R, G, B -> Y, Cb, Cr (src/libsrcnn.cpp:251-256)
__device__ __forceinline__ float split_y(float r, float g, float b) { return (0.299f * r) + (0.587f * g) + (0.114f * b); }
__device__ __forceinline__ float split_cb(float r, float g, float b) { return 128.f - (0.1687f * r) - (0.3313f * g) + (0.5f * b); }
__device__ __forceinline__ float split_cr(float r, float g, float b) { return 128.f + (0.5f * r) - (0.4187f * g) - (0.0813f * b); }

// Y', Cb' - 128, Cr' - 128 -> R, G, B before saturation (src/libsrcnn.cpp:287-307)
__device__ __forceinline__ float merge_r(float fy, float cr) { return fy + 45.f * cr / 32.f; }
__device__ __forceinline__ float merge_g(float fy, float cb, float cr) { return fy - (11.f * cb + 23.f * cr) / 32.f; }
__device__ __forceinline__ float merge_b(float fy, float cb) { return fy + 113.f * cb / 64.f; }

}  // namespace srcnn
