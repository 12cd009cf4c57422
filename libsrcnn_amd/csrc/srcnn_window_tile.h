// srcnn_window_tile.h -- the tile resampler under the window colour kernels of the rect calls: k_rgb_window_merge
// (srcnn_rgb_window.hip), k_yuv_window_chroma (srcnn_yuv_window.hip) and k_yuvp_window_merge (srcnn_yuv_packed_window.hip, whose
// v210 tile is 60 columns wide) resample NC planes of a 64 x 16 tile of the rect straight from the integer source, where the plane
// route (srcnn_window.hip) resamples float planes of the window.
//
// It serves up-scales in both axes with contribution tables of at most 8 taps, where the source patch of every tile fits
// kPatchW x kPatchH: the host asks window_tile_fits, and everything else takes the plane route (srcnn_frames.cpp).  A workgroup
// of 256 threads
//   1. reads the first / last tap of its columns and rows off the tables (LDS min / max): the source patch of the tile
//      (tile_patch),
//   2. stages the NC planes of the patch in LDS as floats (tile_stage); what a source sample's NC floats are is the one part
//      that belongs to the format: a functor of the kernel,
//   3. runs the vertical pass into an fp32 intermediate of 16 rows x patch columns (tile_vertical: the pass order and the
//      rounded intermediate of resample_window for an up-scale),
//   4. runs the horizontal pass for 4 consecutive samples of one row per thread (tile_horizontal gives one of them), and then
//      does with them what the kernel is for.
// Both passes are acc = 0.0; acc = acc + wt[t] * (double)px in tap order; one (float)acc -- the operations of
// k_resample_cols / k_resample_rows, so the tile holds the bits the plane resamplers put at the same place.  The tap count
// of the vertical pass is uniform over a row of the tile; at 2x two neighbouring columns of the horizontal pass read the same
// LDS words (a broadcast), and the 4 rows a wave covers lie kPatchW = 72 words = 8 banks apart.
//
// Every index is bounded: the patch is clamped to the w x h source, and LDS indices lie inside the extents the host checked.
//
// The geometry and the predicate need no HIP (tests/host/yuv_rect_sanitize.cpp runs them on the CPU); the device part is
// compiled by hipcc only.  Internal.
#pragma once
#include <algorithm>

namespace srcnn {

constexpr int kTileW = 64, kTileH = 16;          // the tile of the layer kernels
constexpr int kPatchW = kTileW + 8, kPatchH = kTileH + 8;
constexpr unsigned kTileChunk = 4;               // consecutive samples of one row per thread, in step 4
constexpr int kTileThreads = kTileW * kTileH / (int)kTileChunk;      // 256

// the extent of source indices that `count` destination indices from `start` read, tile by tile of `tile` of them, fits `cap`.
// first / taps: the HOST copies of a contribution table.
inline bool axis_tiles_fit(const int* first, const int* taps, int max_taps, unsigned start, unsigned count, unsigned tile, int cap)
{
    if (!first || !taps || max_taps > 8) return false;
    for (unsigned a = 0; a < count; a += tile) {
        int lo = 0x7fffffff, hi = 0;
        for (unsigned u = start + a; u < start + std::min(count, a + tile); ++u) {
            lo = std::min(lo, first[u]);
            hi = std::max(hi, first[u] + taps[u]);
        }
        if (lo < 0 || hi - lo > cap) return false;
    }
    return true;
}

struct TileAxis {              // what the predicate reads of one table
    const int* first;          // host copies, or NULL
    const int* taps;
    int max_taps;
};

// Whether the tile kernels serve output columns [x0, x0 + cols) and rows [y0, y0 + rows) of the resampled plane: the tables
// (th: columns, tv: rows) have host copies and at most 8 taps, and the source patch of every 64 x 16 tile fits the kernels' LDS.
inline bool window_tile_fits(const TileAxis& th, const TileAxis& tv, unsigned x0, unsigned cols, unsigned y0, unsigned rows)
{
    return axis_tiles_fit(th.first, th.taps, th.max_taps, x0, cols, kTileW, kPatchW) &&
           axis_tiles_fit(tv.first, tv.taps, tv.max_taps, y0, rows, kTileH, kPatchH);
}

}  // namespace srcnn

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "srcnn_kernels.h"

#pragma clang fp contract(off)

namespace srcnn {

inline bool window_tile_fits(const DevAxisTable& th, const DevAxisTable& tv, unsigned x0, unsigned cols, unsigned y0, unsigned rows)
{
    return window_tile_fits(TileAxis{th.h_first, th.h_taps, th.max_taps}, TileAxis{tv.h_first, tv.h_taps, tv.max_taps}, x0, cols, y0, rows);
}

struct TileTables {            // kernel argument: the device side of the two tables
    const int* hf; const int* ht; const double* hw; int hstride;     // horizontal table (output columns <- source columns)
    const int* vf; const int* vt; const double* vw; int vstride;     // vertical table (output rows <- source rows)
};

inline TileTables tile_tables(const DevAxisTable& th, const DevAxisTable& tv)
{
    return TileTables{th.first, th.taps, th.weight, th.stride, tv.first, tv.taps, tv.weight, tv.stride};
}

struct TilePatch {             // the source patch of a tile: its first column and row, its size
    int c_lo, r_lo, pw, ph;
};

// 1. the source patch of the tile whose first sample is (gx, gy) of the output and which has ncol x nrow samples, off the
// tables, clamped to the w x h source.  s_span: int[4] in LDS.  Two barriers.
__device__ __forceinline__ TilePatch tile_patch(const TileTables& a, int* s_span, int tid, unsigned gx, unsigned gy, int ncol, int nrow,
                                                unsigned w, unsigned h)
{
    if (tid == 0) { s_span[0] = 0x7fffffff; s_span[1] = 0; s_span[2] = 0x7fffffff; s_span[3] = 0; }
    __syncthreads();
    if (tid < ncol) {
        const int f = a.hf[gx + tid];
        atomicMin(&s_span[0], f);
        atomicMax(&s_span[1], f + a.ht[gx + tid]);
    } else if (tid >= kTileW && tid - kTileW < nrow) {
        const int f = a.vf[gy + (tid - kTileW)];
        atomicMin(&s_span[2], f);
        atomicMax(&s_span[3], f + a.vt[gy + (tid - kTileW)]);
    }
    __syncthreads();
    const int c_lo = max(s_span[0], 0), r_lo = max(s_span[2], 0);
    const int pw = min(min(s_span[1], (int)w) - c_lo, kPatchW), ph = min(min(s_span[3], (int)h) - r_lo, kPatchH);
    return TilePatch{c_lo, r_lo, pw, ph};
}

// 2. the NC planes of the patch: fetch(source row, source column, float out[NC]).  The caller's barrier follows.
template <int NC, class Fetch>
__device__ __forceinline__ void tile_stage(float (&s_patch)[NC][kPatchH][kPatchW], const TilePatch& p, int tid, Fetch fetch)
{
    for (int i = tid; i < p.pw * p.ph; i += kTileThreads) {
        const int pr = i / p.pw, pc = i - pr * p.pw;
        float v[NC];
        fetch((size_t)(p.r_lo + pr), (size_t)(p.c_lo + pc), v);
#pragma unroll
        for (int k = 0; k < NC; ++k) s_patch[k][pr][pc] = v[k];
    }
}

// 3. vertical pass: rows of the tile x columns of the patch.  The caller's barrier follows.
template <int NC>
__device__ __forceinline__ void tile_vertical(const TileTables& a, const float (&s_patch)[NC][kPatchH][kPatchW],
                                              float (&s_mid)[NC][kTileH][kPatchW], const TilePatch& p, int tid, unsigned gy, int nrow)
{
    for (int i = tid; i < nrow * p.pw; i += kTileThreads) {
        const int ry = i / p.pw, pc = i - ry * p.pw;
        const unsigned y = gy + ry;
        const int s0 = a.vf[y] - p.r_lo, n = a.vt[y];
        const double* wr = a.vw + (size_t)y * a.vstride;
        if (s0 < 0 || s0 + n > kPatchH) continue;            // (never: window_tile_fits)
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            double acc = 0.0;
            for (int t = 0; t < n; ++t) {
                const double px = (double)s_patch[k][s0 + t][pc];
                acc = acc + wr[t] * px;
            }
            s_mid[k][ry][pc] = (float)acc;
        }
    }
}

// 4. horizontal pass: output column x of row ry of the tile, NC planes into rs (left as they are where the taps do not fit)
template <int NC>
__device__ __forceinline__ void tile_horizontal(const TileTables& a, const float (&s_mid)[NC][kTileH][kPatchW], const TilePatch& p, int ry,
                                                unsigned x, float* rs)
{
    const int s0 = a.hf[x] - p.c_lo, nt = a.ht[x];
    const double* wr = a.hw + (size_t)x * a.hstride;
    if (s0 >= 0 && s0 + nt <= kPatchW) {                     // (always: window_tile_fits)
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            double acc = 0.0;
            for (int t = 0; t < nt; ++t) acc = acc + wr[t] * (double)s_mid[k][ry][s0 + t];
            rs[k] = (float)acc;
        }
    }
}

}  // namespace srcnn
#endif  // __HIPCC__
