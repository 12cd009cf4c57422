// srcnn_yuv_packed_merge_tile.h -- the body of the tile merge kernels of packed YUV frames: k_yuvp_window_merge
// (srcnn_yuv_packed_window.hip: one band of one rect per launch) and k_yuvp_list_merge (srcnn_yuv_packed_rect_list.hip: every rect
// of an atlas per launch) instantiate yuvp_merge_tile, as the planar chroma kernels instantiate yuv_chroma_tile
// (srcnn_yuv_chroma_tile.h).  What differs between them is how a workgroup finds its rect and its tile, and where Y' lies: a
// tight band of the rect, or the rect's cell of the layer-3 atlas -- a base pointer and a row stride.  Internal, HIP only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_window_tile.h"
#include "srcnn_yuv_packed_fields.h"

#pragma clang fp contract(off)

namespace srcnn {

struct PkMergeSource {
    const unsigned char* src;                    // the WHOLE frame
    size_t spitch;
    unsigned cw, h;                              // source size on the chroma grid
    TileTables t;                                // horizontal table (dcw <- cw), vertical table (dh <- h)
    YuvPackedRule f;
    int sio;
};

struct PkMergeRect {
    unsigned char* dst;                          // the rect's first byte
    size_t dpitch;
    const float* y;                              // Y' of rows [gy0, gy0 + rows) of the rect's columns: ystride floats per row
    size_t ystride;
    unsigned cx0, gy0;                           // chroma output column of the rect's first column, output row of the first row of y
    unsigned row0;                               // row of the rect at which y starts
    unsigned rw, ccols, rows;                    // luma and chroma columns of the rect, rows of y
    unsigned groups;                             // v210: 16-byte groups of a row segment, the padding groups included
    unsigned blo, bhi;                           // bytes of a source row that may be read
    int dio;
};

namespace {

// the dwords of chunk `c` of a row that lie inside [blo, bhi); the others stay zero
__device__ __forceinline__ void load_chunk(const unsigned char* row, unsigned c, unsigned blo, unsigned bhi, int io, unsigned q[4])
{
    const unsigned b = 16 * c;
    if (io == kIoVec && b >= blo && b + 16 <= bhi) {
        const uint4 x = *reinterpret_cast<const uint4*>(row + b);
        q[0] = x.x; q[1] = x.y; q[2] = x.z; q[3] = x.w;
    } else {
        const int piece = io == kIoVec ? kIoDword : io;
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            q[j] = 0;
            if (b + 4 * j >= blo && b + 4 * j + 4 <= bhi) q[j] = load_dword(row + b + 4 * j, piece);
        }
    }
}

// what an item of yuvp_merge_tile is
template <int K> struct PkItem {
    using S = PkShape<K>;
    static constexpr bool V210 = K == kPkV210;
    static constexpr unsigned CPI = V210 ? 3 : kTileChunk;           // chroma samples of an item
    static constexpr unsigned STEP = S::NY / S::NC;                  // luma samples per chroma sample
    static constexpr unsigned YPI = CPI * STEP;                      // luma samples of an item
    static constexpr unsigned CHUNKS = CPI / S::NC;                  // 16-byte chunks of an item
    static constexpr unsigned TILE = V210 ? 60 : (unsigned)kTileW;   // chroma columns of a tile
    static constexpr unsigned IPR = TILE / CPI;                      // items of a tile's row
    static constexpr int NP = S::NA ? 3 : 2;                         // planes the tile resampler carries
};

// Tile (bx, by) of the chroma grid of rect a (bx * TILE < a.ccols, by * 16 < a.rows: the same for the whole workgroup): U', V'
// (and A') resampled straight from the packed integer source, saturated, put beside Y', converted, encoded by encode<K> and
// stored.  last: the tile is the last of its row of tiles, which for v210 also owns the groups that only pad the row segment.  A
// thread stores only bytes of the rect's span.  Four barriers, no return ahead of the last.
template <int K>
__device__ __forceinline__ void yuvp_merge_tile(const PkMergeSource& s, const PkMergeRect& a, unsigned bx, unsigned by, bool last)
{
    using S = PkShape<K>;
    using I = PkItem<K>;
    constexpr int NP = I::NP;
    __shared__ float s_patch[NP][kPatchH][kPatchW];
    __shared__ float s_mid[NP][kTileH][kPatchW];
    __shared__ int s_span[4];
    const int tid = (int)threadIdx.x;
    const unsigned tx = bx * I::TILE, ty = by * kTileH;                      // the tile inside the rows of y, on the chroma grid
    const int ncol = (int)min(I::TILE, a.ccols - tx), nrow = (int)min((unsigned)kTileH, a.rows - ty);
    const unsigned gx = a.cx0 + tx, gy = a.gy0 + ty;                         // the tile inside the dcw x dh chroma output

    // 1. - 3. (srcnn_window_tile.h); a staged sample is U, V (and A) of a source chroma column: the fields of its chunk
    const TilePatch p = tile_patch(s.t, s_span, tid, gx, gy, ncol, nrow, s.cw, s.h);
    tile_stage<NP>(s_patch, p, tid, [&](size_t sr, size_t sc, float* out) {
        const unsigned c = (unsigned)sc / S::NC, k = (unsigned)sc % S::NC;
        unsigned q[4];
        load_chunk(s.src + sr * s.spitch, c, a.blo, a.bhi, s.sio, q);
        unsigned y[8], u[4], v[4], al[4] = {0, 0, 0, 0};
        decode<K>(q, s.f, y, u, v, al);
        unsigned su = 0, sv = 0, sa = 0;
#pragma unroll
        for (unsigned j = 0; j < S::NC; ++j) {
            su = j == k ? u[j] : su;
            sv = j == k ? v[j] : sv;
            if constexpr (S::NA > 0) sa = j == k ? al[j] : sa;
        }
        out[0] = (float)su;
        out[1] = (float)sv;
        if constexpr (S::NA > 0) out[2] = (float)sa;
    });
    __syncthreads();
    tile_vertical<NP>(s.t, s_patch, s_mid, p, tid, gy, nrow);
    __syncthreads();

    // 4. horizontal pass, saturate, merge with Y', encode, store: one item at a time.  v210: the last tile of a row of tiles also
    // owns the groups that only pad the row segment.
    const float maxv = (float)s.f.mask, amax = (float)s.f.amask;
    unsigned ipr = I::IPR;
    if constexpr (I::V210)
        if (last) ipr = a.groups - bx * I::IPR;
    const unsigned items = (unsigned)nrow * ipr;
    for (unsigned it = (unsigned)tid; it < items; it += kTileThreads) {
        const unsigned ry = it / ipr, c = (it - ry * ipr) * I::CPI;          // row and first chroma column inside the tile
        const unsigned n = c < (unsigned)ncol ? min(I::CPI, (unsigned)ncol - c) : 0u;    // chroma samples of the item
        if (!I::V210 && n == 0) continue;
        const size_t br = (size_t)ty + ry;                       // row of y
        const size_t dr = (size_t)a.row0 + br;                   // row of the rect = destination row
        const unsigned dc = tx + c;                              // chroma column of the rect
        const unsigned y0 = I::STEP * dc;                        // luma column of the rect
        const unsigned ny = y0 < a.rw ? min(I::YPI, a.rw - y0) : 0u;
        unsigned y[I::YPI], u[I::CPI], v[I::CPI], al[I::CPI];
#pragma unroll
        for (unsigned k = 0; k < I::CPI; ++k) {
            float rs[3] = {0.f, 0.f, 0.f};
            if (k < n) tile_horizontal<NP>(s.t, s_mid, p, (int)ry, gx + c + k, rs);
            u[k] = k < n ? to_word<true>(rs[0], 1.f, maxv) : 0u;
            v[k] = k < n ? to_word<true>(rs[1], 1.f, maxv) : 0u;
            al[k] = (S::NA > 0 && k < n) ? to_word<true>(rs[2], 1.f, amax) : 0u;
        }
#pragma unroll
        for (unsigned k = 0; k < I::YPI; ++k) {
            float fy = 0.f;
            if (k < ny) fy = a.y[br * a.ystride + y0 + k];
            y[k] = k < ny ? to_word<false>(fy, s.f.up, maxv) : 0u;
        }
        unsigned q[4 * I::CHUNKS];
#pragma unroll
        for (unsigned j = 0; j < I::CHUNKS; ++j) encode<K>(y + j * S::NY, u + j * S::NC, v + j * S::NC, al + j * S::NC, s.f, q + 4 * j);
        // dwords of the item that belong to the span: a chroma sample of the 4:2:2 and 4:4:4 kinds is 1 or 2 dwords; v210: the group
        const unsigned nd = I::V210 ? 4u : n * (4 * I::CHUNKS / I::CPI);
        unsigned char* d = a.dst + dr * a.dpitch + (size_t)(dc / I::CPI) * (16 * I::CHUNKS);
        if (nd == 4 * I::CHUNKS && a.dio == kIoVec) {
#pragma unroll
            for (unsigned j = 0; j < I::CHUNKS; ++j)
                *reinterpret_cast<uint4*>(d + 16 * j) = make_uint4(q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]);
        } else {
            const int piece = a.dio == kIoVec ? kIoDword : a.dio;
#pragma unroll
            for (unsigned j = 0; j < 4 * I::CHUNKS; ++j)
                if (j < nd) store_dword(d + 4 * j, q[j], piece);
        }
    }
}

}  // namespace

}  // namespace srcnn
