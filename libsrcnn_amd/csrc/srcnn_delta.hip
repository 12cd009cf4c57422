// srcnn_delta.hip -- the delta calls' kernels (include/srcnn_amd_delta.h, include/srcnn_amd_rgb_delta.h): which tiles of the
// output can differ between two source surfaces.  The contract and the span tables are srcnn_delta.hpp's and srcnn_rgb_delta.hpp's.
#include "srcnn_delta.h"

#include <stdint.h>

#include <algorithm>

#include "srcnn_delta.hpp"
#include "srcnn_pixel_io.h"

namespace srcnn {

// The frame of both kernels.  Source-driven: every unit (a word of the float plane, a byte of a pixel surface) of both surfaces
// is read exactly once, where a kernel that walked the output tiles would read the tap and halo overlap of neighbouring tiles
// again.  A work item is one piece of one source row; workgroups stride over the items.  A chunk is 16 bytes; a lane's chunks
// are 256 lanes apart, so that a wave's loads are contiguous.  Every load is unconditional -- a lane whose chunk lies past the
// row's end reads the row's last whole chunk (last unit) again and drops the result -- so that all loads of an item are in
// flight before the first compare.  VEC (decided once per launch: bases and pitches multiples of 16, a row of at least one
// chunk): a whole chunk is one 16-byte load from each surface, the row's partial chunk is read by the one lane it falls to
// (delta_no_tail); otherwise every unit is a load of its own.  Nothing between a row's end and the pitch is ever read.
//
// Exactness.  Comparison is on the bit patterns.  A chunk with a differing unit is examined unit by unit: the tile columns whose
// span holds source column x are [#{c : xhi[c] <= x}, #{c : xlo[c] <= x}), two bisections of the monotone tables in LDS, and
// every one of them gets a hit byte in LDS (delta_mark).  The tile rows are found the same way from the row, once per item, by
// every lane alike.  After the barrier the hit columns are stored: the byte 1 into flags[r * cols + c], a plain store -- every
// writer of a flag stores the same value, so there is nothing to order -- and the hit bytes are cleared for the next item
// (delta_store_item).  An item without a differing unit costs its loads, the compares and one barrier.
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

// A workgroup's LDS: the span tables xlo[cols], xhi[cols], ylo[rows], yhi[rows], then a hit byte per column
extern __shared__ unsigned s_tab[];
struct DeltaTables { const unsigned *xlo, *xhi, *ylo, *yhi; unsigned char* hit; };

// the image of the tables copied, the hit bytes clear, and every lane past the barrier
__device__ __forceinline__ DeltaTables delta_tables(const unsigned* spans, unsigned cols, unsigned rows, unsigned tid)
{
    const DeltaTables t{s_tab, s_tab + cols, s_tab + cols + cols, s_tab + cols + cols + rows, reinterpret_cast<unsigned char*>(s_tab + 2 * (cols + rows))};
    for (unsigned i = tid; i < 2 * (cols + rows); i += kDeltaThreads) s_tab[i] = spans[i];
    for (unsigned i = tid; i < cols; i += kDeltaThreads) t.hit[i] = 0;
    __syncthreads();
    return t;
}

// This lane has NO partial chunk to read: the row has none, or chunk `whole` is not in this piece of CHUNKS chunks, or not this
// lane's.  (The form that compiles to what the condition gave written out in each kernel: profiles/delta_frame_isa.txt.)
template <unsigned CHUNKS>
__device__ __forceinline__ bool delta_no_tail(unsigned tail, unsigned whole, unsigned piece, unsigned ch0)
{
    return !tail || whole < piece * CHUNKS || whole >= (piece + 1) * CHUNKS || (whole - ch0) % kDeltaThreads != 0;
}

// the end of an item of source row y: the hit columns into the flags of the row's tile rows
__device__ __forceinline__ void delta_store_item(const DeltaTables& t, int any, unsigned y, unsigned cols, unsigned rows, unsigned tid, unsigned char* flags)
{
    if (__syncthreads_or(any)) {                          // the same answer in every lane
        const unsigned r1 = delta_count_le(t.ylo, rows, y);
        const unsigned r0 = delta_count_le(t.yhi, rows, y);
        for (unsigned c = tid; c < cols; c += kDeltaThreads) {
            if (!t.hit[c]) continue;
            t.hit[c] = 0;
            for (unsigned r = r0; r < r1; ++r) flags[(size_t)r * cols + c] = 1;
        }
        __syncthreads();                                  // the hit bytes are clear before the next item marks them
    }
}

// What both launchers do with their instance: the flags cleared, the LDS bytes, the capped grid.  surface: its leading arguments
template <class Kernel, class... Surface>
static void delta_launch(Kernel k, hipStream_t s, unsigned pieces, unsigned items, const unsigned* d_spans, unsigned cols, unsigned rows,
                         unsigned char* d_flags, Surface... surface)
{
    (void)hipMemsetAsync(d_flags, 0, (size_t)cols * rows, s);
    const size_t lds = sizeof(unsigned) * delta_span_words(cols, rows) + ((size_t)cols + 3) / 4 * 4;
    hipLaunchKernelGGL(k, dim3(std::min(items, kDeltaGridCap)), dim3(kDeltaThreads), lds, s, surface..., pieces, items, d_spans, cols, rows, d_flags);
}

// =====================================================================================================================
// k_delta_flags
// =====================================================================================================================
// The float plane: 8 * w * h bytes in all.  A unit is a 32-bit word; a lane compares kDeltaUnroll chunks of 4 floats, a piece is
// kDeltaPiece floats.  Without VEC every word is a load of its own.  A chunk that differs is a mask of its 4 words.
template <bool VEC>
__global__ __launch_bounds__(kDeltaThreads) void k_delta_flags(const unsigned char* __restrict__ prev, size_t prev_pitch,
                                                                const unsigned char* __restrict__ cur, size_t cur_pitch, unsigned w,
                                                                unsigned pieces, unsigned items, const unsigned* __restrict__ spans,
                                                                unsigned cols, unsigned rows, unsigned char* __restrict__ flags)
{
    const unsigned tid = threadIdx.x;
    const DeltaTables t = delta_tables(spans, cols, rows, tid);
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
            delta_mark(t.xlo, t.xhi, cols, 4 * (ch0 + (bit >> 2) * kDeltaThreads) + (bit & 3u), t.hit);
        }
        if constexpr (VEC) {                              // the row's partial chunk, for the lane whose chunk it would be
            if (!delta_no_tail<kDeltaPiece / 4>(tail, whole, piece, ch0)) {
                for (unsigned k = 0; k < tail; ++k)
                    if (p[4 * whole + k] != q[4 * whole + k]) { any = 1; delta_mark(t.xlo, t.xhi, cols, 4 * whole + k, t.hit); }
            }
        }
        delta_store_item(t, any, y, cols, rows, tid, flags);
    }
}

void launch_delta_flags(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h,
                        const unsigned* d_spans, unsigned cols, unsigned rows, unsigned char* d_flags, hipStream_t s)
{
    const unsigned pieces = (w + kDeltaPiece - 1) / kDeltaPiece;
    const unsigned items = pieces * h;                    // (w * h < 2^31 and h <= 2^20: no overflow)
    const unsigned char *p = reinterpret_cast<const unsigned char*>(d_prev), *q = reinterpret_cast<const unsigned char*>(d_cur);
    const bool vec = w >= 4 && aligned_to(d_prev, 16) && aligned_to(d_cur, 16) && prev_pitch % 16 == 0 && cur_pitch % 16 == 0;
    delta_launch(vec ? k_delta_flags<true> : k_delta_flags<false>, s, pieces, items, d_spans, cols, rows, d_flags, p, prev_pitch, q, cur_pitch, w);
}

// =====================================================================================================================
// k_delta_flags_bytes
// =====================================================================================================================
// Integer pixel surfaces (include/srcnn_amd_rgb_delta.h): up to four planes that share one pixel grid, one pair of span tables
// (in PIXELS) and one set of hit bytes.  A unit is a byte; a pixel is bpp consecutive bytes of a plane's row (3, 4, 6 or 8
// interleaved, 1 or 2 planar), so the pixel of byte b of a row is b / bpp, whatever word, chunk or piece b is in.  A work item is
// one piece of one row of one plane, items = planes * h * pieces; a lane compares U chunks, a piece is 256 * U chunks.
// The piece.  These rows are short next to the float plane's: 11 520 B (720 chunks) for 3840 RGB8 pixels, 15 360 B (960) for
// BGRA, 5 760 B (360) for 1920 RGB8.  A fixed piece of 1024 chunks would leave 30 % of the lanes of every RGB8 item without a
// chunk, a fixed piece of 256 would leave the 960-chunk row with two loads in flight per lane where eight fit.  So U is a
// template parameter, 1 ... 4, and the launcher takes the U that pads the row's chunks least and, among those, the largest:
// 720 -> U = 3 (768), 960 -> U = 4 (1024), 360 -> U = 2 (512), 480 -> U = 2 (512), 240 -> U = 1 (256).
//
// VEC (with one row the pitches place nothing and need not be multiples of 16): the row's last row_bytes % 16 bytes are read in
// words and then bytes.  Otherwise (depth 8 allows odd bases and pitches) every byte is a load of its own, clamped to the row's
// last byte: correct at any alignment, one instance (U = 1), not fast.
// The compare.  The clean path ORs the XORs of a chunk's four words.  A chunk that differs is taken apart into a mask of its
// differing BYTES; every such byte's pixel, b / bpp (a division, on this rare path), gets its tile columns marked.  A pixel that
// merely shares a word or a chunk with a differing byte is not marked; a pixel that straddles a word, a chunk or a piece is
// marked by whichever lane or item sees one of its bytes differ, to the same columns.
__device__ __forceinline__ unsigned delta_byte_mask(unsigned x)          // bit j: byte j of the word is not 0
{
    return (x & 0xffu ? 1u : 0u) | (x & 0xff00u ? 2u : 0u) | (x & 0xff0000u ? 4u : 0u) | (x & 0xff000000u ? 8u : 0u);
}

template <bool VEC, int U>
__global__ __launch_bounds__(kDeltaThreads) void k_delta_flags_bytes(const DeltaBytePlanes P, unsigned pieces, unsigned items,
                                                                      const unsigned* __restrict__ spans, unsigned cols, unsigned rows,
                                                                      unsigned char* __restrict__ flags)
{
    const unsigned tid = threadIdx.x;
    const DeltaTables t = delta_tables(spans, cols, rows, tid);
    const unsigned whole = P.row_bytes / 16, tail = P.row_bytes % 16;      // whole chunks of a row, bytes of its partial chunk
    const unsigned per_plane = P.rows * pieces;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned plane = item / per_plane, in_plane = item - plane * per_plane;
        const unsigned y = in_plane / pieces, piece = in_plane - y * pieces;
        const unsigned char* p = P.prev[plane] + (size_t)y * P.prev_pitch[plane];
        const unsigned char* q = P.cur[plane] + (size_t)y * P.cur_pitch[plane];
        const unsigned ch0 = piece * (unsigned)(U * kDeltaThreads) + tid;
        unsigned long long mm = 0;                        // bit 16 * u + j: byte j of chunk u differs
        if constexpr (VEC) {
            uint4 a[U], b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned ch = min(ch0 + (unsigned)u * kDeltaThreads, whole - 1);      // (row_bytes >= 16: the launcher)
                a[u] = *reinterpret_cast<const uint4*>(p + 16 * (size_t)ch);
                b[u] = *reinterpret_cast<const uint4*>(q + 16 * (size_t)ch);
            }
            unsigned d = 0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned x = (a[u].x ^ b[u].x) | (a[u].y ^ b[u].y) | (a[u].z ^ b[u].z) | (a[u].w ^ b[u].w);
                d |= ch0 + (unsigned)u * kDeltaThreads < whole ? x : 0u;
            }
            if (d) {                                      // (rare: which bytes)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const unsigned m = delta_byte_mask(a[u].x ^ b[u].x) | delta_byte_mask(a[u].y ^ b[u].y) << 4 |
                                       delta_byte_mask(a[u].z ^ b[u].z) << 8 | delta_byte_mask(a[u].w ^ b[u].w) << 12;
                    if (ch0 + (unsigned)u * kDeltaThreads < whole) mm |= (unsigned long long)m << (16 * u);
                }
            }
        } else {
            unsigned char a[U][16], b[U][16];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const unsigned at = min(16 * (ch0 + (unsigned)u * kDeltaThreads) + (unsigned)j, P.row_bytes - 1);
                    a[u][j] = p[at];
                    b[u][j] = q[at];
                }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (16 * (ch0 + (unsigned)u * kDeltaThreads) + (unsigned)j < P.row_bytes && a[u][j] != b[u][j]) mm |= 1ull << (16 * u + j);
        }
        int any = mm != 0;
        unsigned last = ~0u;                              // (bytes of one pixel follow each other: one mark per pixel)
        while (mm) {                                      // (rare, and not unrolled: the clean path is a branch over it)
            const unsigned bit = (unsigned)__ffsll((long long)mm) - 1u;
            mm &= mm - 1ull;
            const unsigned x = (16 * (ch0 + (bit >> 4) * kDeltaThreads) + (bit & 15u)) / P.bpp;
            if (x != last) delta_mark(t.xlo, t.xhi, cols, x, t.hit);
            last = x;
        }
        if constexpr (VEC) {                              // the row's partial chunk, for the lane whose chunk it would be
            if (!delta_no_tail<(unsigned)(U * kDeltaThreads)>(tail, whole, piece, ch0)) {
                const unsigned at = 16 * whole;           // (a multiple of 16 from a 16-byte aligned row: words are aligned)
                unsigned k = 0;
                for (; k + 4 <= tail; k += 4) {
                    const unsigned m = delta_byte_mask(*reinterpret_cast<const unsigned*>(p + at + k) ^ *reinterpret_cast<const unsigned*>(q + at + k));
                    for (unsigned j = 0; j < 4; ++j)
                        if (m >> j & 1u) { any = 1; delta_mark(t.xlo, t.xhi, cols, (at + k + j) / P.bpp, t.hit); }
                }
                for (; k < tail; ++k)
                    if (p[at + k] != q[at + k]) { any = 1; delta_mark(t.xlo, t.xhi, cols, (at + k) / P.bpp, t.hit); }
            }
        }
        delta_store_item(t, any, y, cols, rows, tid, flags);
    }
}

void launch_delta_flags_bytes(const DeltaBytePlanes& P, const unsigned* d_spans, unsigned cols, unsigned rows, unsigned char* d_flags, hipStream_t s)
{
    bool vec = P.row_bytes >= 16;
    for (unsigned k = 0; k < P.planes; ++k)
        vec = vec && aligned_to(P.prev[k], 16) && aligned_to(P.cur[k], 16) &&
              (P.rows == 1 || (P.prev_pitch[k] % 16 == 0 && P.cur_pitch[k] % 16 == 0));      // (one row: the pitch places nothing)
    const unsigned chunks = (P.row_bytes + 15) / 16;
    unsigned unroll = 1, padded = ~0u;                    // the U that pads the row least; among those the largest
    for (unsigned u = 1; vec && u <= 4; ++u) {
        const unsigned span = u * kDeltaThreads, n = (chunks + span - 1) / span * span;
        if (n <= padded) { padded = n; unroll = u; }
    }
    const unsigned pieces = (chunks + unroll * kDeltaThreads - 1) / (unroll * kDeltaThreads);
    const unsigned items = P.planes * P.rows * pieces;    // (row_bytes * rows < 2^34 over all planes: under 2^23)
    const auto k = !vec ? k_delta_flags_bytes<false, 1> : unroll == 1 ? k_delta_flags_bytes<true, 1> : unroll == 2 ? k_delta_flags_bytes<true, 2> :
                   unroll == 3 ? k_delta_flags_bytes<true, 3> : k_delta_flags_bytes<true, 4>;
    delta_launch(k, s, pieces, items, d_spans, cols, rows, d_flags, P);
}

}  // namespace srcnn
