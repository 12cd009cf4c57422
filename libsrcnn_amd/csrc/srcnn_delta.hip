// srcnn_delta.hip -- the delta call's kernel (include/srcnn_amd_delta.h): which tiles of the output can differ between two
// source planes.  The contract and the span tables are srcnn_delta.hpp's.
#include "srcnn_delta.h"

#include <stdint.h>

#include <algorithm>

#include "srcnn_delta.hpp"
#include "srcnn_pixel_io.h"

namespace srcnn {

// =====================================================================================================================
// k_delta_flags
// =====================================================================================================================
// Source-driven: every sample of both planes is read exactly once, 8 * w * h bytes in all, where a kernel that walked the output
// tiles would read the tap and halo overlap of neighbouring tiles again.  A work item is one piece of kDeltaPiece floats of
// one source row; workgroups stride over the items.  A lane compares kDeltaUnroll chunks of 4 floats, 256 lanes apart so that a
// wave's loads are contiguous.  Every load is unconditional -- a lane whose chunk lies past the row's end reads the row's last
// whole chunk (last word) again and drops the result -- so that all loads of an item are in flight before the first compare.
// VEC (both bases and both pitches multiples of 16 and w >= 4, decided once per launch): a whole chunk is one 16-byte load from
// each plane, and the last partial chunk of a row is read word by word by the one lane it falls to; otherwise every word is a
// load of its own.  Nothing between a row's w floats and the pitch is ever read.
//
// Exactness.  Comparison is on the 32-bit patterns.  A chunk with a differing word is examined word by word: the tile columns
// whose span holds source column x are [#{c : xhi[c] <= x}, #{c : xlo[c] <= x}), two bisections of the monotone tables in LDS,
// and every one of them gets a hit byte in LDS.  The tile rows are found the same way from the row, once per item, by every
// lane alike.  After the barrier the hit columns are stored: the byte 1 into flags[r * cols + c], a plain store -- every
// writer of a flag stores the same value, so there is nothing to order -- and the hit bytes are cleared for the next item.
// An item without a differing word costs its loads, the compares and one barrier.
constexpr int kDeltaThreads = 256;
constexpr int kDeltaUnroll = 4;
constexpr unsigned kDeltaPiece = kDeltaThreads * kDeltaUnroll * 4;      // floats of a row per work item
constexpr unsigned kDeltaGridCap = 2048;                                // 256 CUs x 8 workgroups; the rest is strided

// #{k < n : t[k] <= x}, t non-decreasing
__device__ __forceinline__ unsigned delta_count_le(const unsigned* t, unsigned n, unsigned x)
{
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (t[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// a hit byte for every tile column whose span holds source column x
__device__ __forceinline__ void delta_mark(const unsigned* xlo, const unsigned* xhi, unsigned cols, unsigned x, unsigned char* hit)
{
    const unsigned c1 = delta_count_le(xlo, cols, x);
    for (unsigned c = delta_count_le(xhi, cols, x); c < c1; ++c) hit[c] = 1;
}

template <bool VEC>
__global__ __launch_bounds__(kDeltaThreads) void k_delta_flags(const unsigned char* __restrict__ prev, size_t prev_pitch,
                                                                const unsigned char* __restrict__ cur, size_t cur_pitch, unsigned w,
                                                                unsigned pieces, unsigned items, const unsigned* __restrict__ spans,
                                                                unsigned cols, unsigned rows, unsigned char* __restrict__ flags)
{
    extern __shared__ unsigned s_tab[];                   // xlo[cols], xhi[cols], ylo[rows], yhi[rows], then a hit byte per column
    const unsigned* xlo = s_tab;
    const unsigned* xhi = xlo + cols;
    const unsigned* ylo = xhi + cols;
    const unsigned* yhi = ylo + rows;
    unsigned char* hit = reinterpret_cast<unsigned char*>(s_tab + 2 * (cols + rows));
    const unsigned tid = threadIdx.x;
    for (unsigned i = tid; i < 2 * (cols + rows); i += kDeltaThreads) s_tab[i] = spans[i];
    for (unsigned i = tid; i < cols; i += kDeltaThreads) hit[i] = 0;
    __syncthreads();

    const unsigned whole = w / 4, tail = w % 4;           // whole chunks of a row, words of its partial chunk
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned y = item / pieces, piece = item - y * pieces;
        const unsigned* p = reinterpret_cast<const unsigned*>(prev + (size_t)y * prev_pitch);
        const unsigned* q = reinterpret_cast<const unsigned*>(cur + (size_t)y * cur_pitch);
        const unsigned ch0 = piece * (kDeltaPiece / 4) + tid;
        unsigned m[kDeltaUnroll];                         // bit k: word k of chunk u differs
        if constexpr (VEC) {
            uint4 a[kDeltaUnroll], b[kDeltaUnroll];
#pragma unroll
            for (int u = 0; u < kDeltaUnroll; ++u) {
                const unsigned ch = min(ch0 + (unsigned)u * kDeltaThreads, whole - 1);      // (w >= 4: the launcher)
                a[u] = *reinterpret_cast<const uint4*>(p + 4 * ch);
                b[u] = *reinterpret_cast<const uint4*>(q + 4 * ch);
            }
#pragma unroll
            for (int u = 0; u < kDeltaUnroll; ++u) {
                const unsigned d = (a[u].x != b[u].x ? 1u : 0u) | (a[u].y != b[u].y ? 2u : 0u) | (a[u].z != b[u].z ? 4u : 0u) | (a[u].w != b[u].w ? 8u : 0u);
                m[u] = ch0 + (unsigned)u * kDeltaThreads < whole ? d : 0u;
            }
        } else {
            unsigned a[kDeltaUnroll][4], b[kDeltaUnroll][4];
#pragma unroll
            for (int u = 0; u < kDeltaUnroll; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned x = min(4 * (ch0 + (unsigned)u * kDeltaThreads) + (unsigned)k, w - 1);
                    a[u][k] = p[x];
                    b[u][k] = q[x];
                }
#pragma unroll
            for (int u = 0; u < kDeltaUnroll; ++u) {
                m[u] = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * (ch0 + (unsigned)u * kDeltaThreads) + (unsigned)k < w && a[u][k] != b[u][k]) m[u] |= 1u << k;
            }
        }
        unsigned mm = 0;                                  // bit 4 * u + k: word k of chunk u differs
#pragma unroll
        for (int u = 0; u < kDeltaUnroll; ++u) mm |= m[u] << (4 * u);
        int any = mm != 0;
        while (mm) {                                      // (rare, and not unrolled: the clean path is a branch over it)
            const unsigned bit = (unsigned)__ffs((int)mm) - 1u;
            mm &= mm - 1u;
            delta_mark(xlo, xhi, cols, 4 * (ch0 + (bit >> 2) * kDeltaThreads) + (bit & 3u), hit);
        }
        if constexpr (VEC) {                              // the row's partial chunk, for the lane whose chunk it would be
            if (tail && whole >= piece * (kDeltaPiece / 4) && whole < (piece + 1) * (kDeltaPiece / 4) && (whole - ch0) % kDeltaThreads == 0) {
                for (unsigned k = 0; k < tail; ++k)
                    if (p[4 * whole + k] != q[4 * whole + k]) { any = 1; delta_mark(xlo, xhi, cols, 4 * whole + k, hit); }
            }
        }
        if (__syncthreads_or(any)) {                      // the same answer in every lane
            const unsigned r1 = delta_count_le(ylo, rows, y);
            const unsigned r0 = delta_count_le(yhi, rows, y);
            for (unsigned c = tid; c < cols; c += kDeltaThreads) {
                if (!hit[c]) continue;
                hit[c] = 0;
                for (unsigned r = r0; r < r1; ++r) flags[(size_t)r * cols + c] = 1;
            }
            __syncthreads();                              // the hit bytes are clear before the next item marks them
        }
    }
}

void launch_delta_flags(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h,
                        const unsigned* d_spans, unsigned cols, unsigned rows, unsigned char* d_flags, hipStream_t s)
{
    (void)hipMemsetAsync(d_flags, 0, (size_t)cols * rows, s);
    const unsigned pieces = (w + kDeltaPiece - 1) / kDeltaPiece;
    const unsigned items = pieces * h;                    // (w * h < 2^31 and h <= 2^20: no overflow)
    const size_t lds = sizeof(unsigned) * delta_span_words(cols, rows) + ((size_t)cols + 3) / 4 * 4;
    const dim3 g(std::min(items, kDeltaGridCap));
    const unsigned char* p = reinterpret_cast<const unsigned char*>(d_prev);
    const unsigned char* q = reinterpret_cast<const unsigned char*>(d_cur);
    const bool vec = w >= 4 && aligned_to(d_prev, 16) && aligned_to(d_cur, 16) && prev_pitch % 16 == 0 && cur_pitch % 16 == 0;
    if (vec) hipLaunchKernelGGL((k_delta_flags<true>), g, dim3(kDeltaThreads), lds, s, p, prev_pitch, q, cur_pitch, w, pieces, items, d_spans, cols, rows, d_flags);
    else hipLaunchKernelGGL((k_delta_flags<false>), g, dim3(kDeltaThreads), lds, s, p, prev_pitch, q, cur_pitch, w, pieces, items, d_spans, cols, rows, d_flags);
}

}  // namespace srcnn
