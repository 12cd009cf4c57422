// srcnn_yuv_rect_list.hip -- the three kernels that join planar / semi-planar YUV frames to the atlas of the rect LIST call
// (include/srcnn_amd_yuv_rect_list.h).  Between the first and the other two run the list's own launches, unchanged
// (srcnn_rect_list.hip and the layer kernels).
//
//   k_yuv_list_resample   k_list_resample with an integer fetch: the in-plane part of every cell, resampled by the tile
//                         resampler straight from the caller's luma plane with the luma read rule of k_plane_unpack
//                         (srcnn_yuv_planes.hip): (float)byte, or (float)word_value(word, rshift, mask) * down.  No float plane
//                         of the source frame exists.
//   k_yuv_list_luma       k_list_scatter's place: one workgroup takes one 64 x 16 tile of one rect, found by bisection over
//                         sc_tile0, reads Y' from the layer-3 atlas and stores it into the item's luma plane with the luma write
//                         rule of k_plane_pack (not saturated: layer 3 clamps; (unsigned char)v, or (unsigned)(v * up) << lshift).
//                         A thread's 4 samples go out as one 4- / 8-byte store where that item's base and pitch allow it.
//   k_yuv_list_chroma     one workgroup takes one 64 x 16 tile of one item's CHROMA rect, found by bisection over ch_tile0 of the
//                         destination table (YuvListDstDesc, srcnn_yuv_rect_atlas.hpp), and runs yuv_chroma_tile
//                         (srcnn_yuv_chroma_tile.h), the body of k_yuv_window_chroma, with the vector-store flag of that item.
//
// Luma and chroma are two launches: their grids differ (rect tiles against chroma-rect tiles), the luma kernel needs no LDS and
// no barrier, and the chroma kernel does not wait for the layers.  The pixel rules are srcnn_colour_rules.h.
//
// Every index is bounded: a tile is cut to its rect (chroma rect), the source patch is clamped to the plane (tile_patch), the cell
// lies inside the atlas (tests/host/rect_list_sanitize.cpp), and a thread stores only samples of its own rect: rw (ccols) per
// row, rh (crows) rows (tests/host/yuv_rect_list_sanitize.cpp recomputes that range off the descriptors).  Every return ahead
// of a barrier depends on the workgroup's cell and tile alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_rect_list.h"
#include "srcnn_window_tile.h"
#include "srcnn_yuv.h"
#include "srcnn_yuv_chroma_tile.h"
#include "srcnn_yuv_rect_atlas.hpp"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr int kCols = kTileW / (int)kTileChunk;      // threads per tile row

struct YuvListResample {
    const unsigned char* sp;                     // the WHOLE source luma plane
    size_t spitch;
    unsigned w, h;
    unsigned rshift, mask;
    float down;
    TileTables t;                                // the Y tables: horizontal (dw <- w), vertical (dh <- h)
    const ListCellDesc* d;
    unsigned n;
    float* atlas;
    unsigned atlas_w;
};

struct YuvListLuma {
    const ListCellDesc* d;
    const YuvListDstDesc* dd;                    // entry k: the destination of cell k
    unsigned n;
    const float* atlas;                          // the layer-3 result
    unsigned atlas_w;
    float up;
    unsigned lshift;
};

struct YuvListChroma {
    ChromaTileSource src;
    const YuvListDstDesc* dd;
    unsigned n;
};

template <int BPS>
__global__ __launch_bounds__(256) void k_yuv_list_resample(const YuvListResample a)
{
    list_resample_tile(a.w, a.h, a.t, a.d, a.n, a.atlas, a.atlas_w, [&](size_t sr, size_t sc, float* v) {
        const unsigned char* q = a.sp + sr * a.spitch + sc * BPS;
        if constexpr (BPS == 1) v[0] = (float)load_scalar<1>(q);
        else v[0] = (float)word_value(load_scalar<2>(q), a.rshift, a.mask) * a.down;
    });
}

template <int BPS>
__global__ __launch_bounds__(256) void k_yuv_list_luma(const YuvListLuma a)
{
    const int tid = (int)threadIdx.x;
    const unsigned cell = find_cell<&ListCellDesc::sc_tile0>(a.d, a.n, blockIdx.x);
    const ListCellDesc c = a.d[cell];
    const unsigned tile = blockIdx.x - c.sc_tile0, tiles_x = (c.rw + kTileW - 1) / kTileW;
    const unsigned y = (tile / tiles_x) * kTileH + tid / kCols;                          // row of the rect
    const unsigned x = (tile % tiles_x) * kTileW + (tid % kCols) * kTileChunk;           // first of this thread's columns
    if (y >= c.rh || x >= c.rw) return;
    const float* in = a.atlas + (size_t)(c.ay + kCellMargin + y) * a.atlas_w + (c.ax + kCellMargin + x);
    const YuvListDstDesc o = a.dd[cell];
    unsigned char* out = reinterpret_cast<unsigned char*>((uintptr_t)o.plane[0]) + (size_t)y * o.pitch[0] + (size_t)x * BPS;
    const unsigned nn = min(kTileChunk, c.rw - x);
    unsigned code[kTileChunk];
#pragma unroll
    for (unsigned k = 0; k < kTileChunk; ++k) {
        const float v = k < nn ? in[k] : 0.f;
        if constexpr (BPS == 1) code[k] = (unsigned char)v;
        else code[k] = (unsigned)(v * a.up) << a.lshift;
    }
    if (nn == kTileChunk && o.luma_vec) {                    // (x is a multiple of 4: the store is aligned with base and pitch)
        unsigned wd[BPS] = {};
#pragma unroll
        for (unsigned k = 0; k < kTileChunk; ++k) put_sample<BPS>(wd, (int)k, code[k]);
        store_chunk<BPS>(out, wd);
    } else {
#pragma unroll
        for (unsigned k = 0; k < kTileChunk; ++k)
            if (k < nn) store_scalar<BPS>(out + (size_t)k * BPS, code[k]);
    }
}

// the largest k < n with dd[k].ch_tile0 <= b (dd[0].ch_tile0 == 0, and b is below the total)
__device__ __forceinline__ unsigned find_chroma_entry(const YuvListDstDesc* __restrict__ dd, unsigned n, unsigned b)
{
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (dd[mid].ch_tile0 <= b) lo = mid; else hi = mid;
    }
    return lo;
}

template <int BPS, bool SEMI>
__global__ __launch_bounds__(256) void k_yuv_list_chroma(const YuvListChroma a)
{
    const YuvListDstDesc o = a.dd[find_chroma_entry(a.dd, a.n, blockIdx.x)];             // the same for the whole workgroup
    const unsigned tile = blockIdx.x - o.ch_tile0, tiles_x = (o.ccols + kTileW - 1) / kTileW;
    const unsigned tx = (tile % tiles_x) * kTileW, ty = (tile / tiles_x) * kTileH;       // the tile inside the chroma rect
    if (tx >= o.ccols || ty >= o.crows) return;                                          // (never: the prefix sum counts these tiles)
    ChromaTileDst d;
    d.dp[0] = reinterpret_cast<unsigned char*>((uintptr_t)o.plane[1]);
    d.dp[1] = reinterpret_cast<unsigned char*>((uintptr_t)o.plane[2]);
    d.dpitch[0] = o.pitch[1]; d.dpitch[1] = o.pitch[2];
    d.cx0 = o.cx0; d.cy0 = o.cy0; d.cols = o.ccols; d.rows = o.crows;
    d.dst_vec = (int)o.chroma_vec;
    yuv_chroma_tile<BPS, SEMI>(a.src, d, tx, ty);
}

}  // namespace

void launch_yuv_list_resample(const unsigned char* src, size_t spitch, unsigned w, unsigned h, const Yuv16Rule* f, const DevAxisTable& th,
                              const DevAxisTable& tv, const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas,
                              unsigned atlas_w, hipStream_t s)
{
    if (ncells == 0 || end.rs_tile0 == 0) return;
    const YuvListResample a{src, spitch, w, h, f ? f->rshift : 0, f ? f->mask : 0xffu, f ? f->down : 1.f, tile_tables(th, tv), d, ncells, atlas, atlas_w};
    if (f) hipLaunchKernelGGL(k_yuv_list_resample<2>, dim3(end.rs_tile0), dim3(kTileThreads), 0, s, a);
    else hipLaunchKernelGGL(k_yuv_list_resample<1>, dim3(end.rs_tile0), dim3(kTileThreads), 0, s, a);
}

void launch_yuv_list_luma(const Yuv16Rule* f, const ListCellDesc* d, const YuvListDstDesc* dd, unsigned ncells, const ListCellDesc& end,
                          const float* atlas, unsigned atlas_w, hipStream_t s)
{
    if (ncells == 0 || end.sc_tile0 == 0) return;
    const YuvListLuma a{d, dd, ncells, atlas, atlas_w, f ? f->up : 1.f, f ? f->lshift : 0};
    if (f) hipLaunchKernelGGL(k_yuv_list_luma<2>, dim3(end.sc_tile0), dim3(kTileThreads), 0, s, a);
    else hipLaunchKernelGGL(k_yuv_list_luma<1>, dim3(end.sc_tile0), dim3(kTileThreads), 0, s, a);
}

void launch_yuv_list_chroma(const unsigned char* const src[2], const size_t spitch[2], unsigned cw, unsigned ch, bool semi, const Yuv16Rule* f,
                            const DevAxisTable& cth, const DevAxisTable& ctv, const YuvListDstDesc* dd, unsigned ncells,
                            const YuvListDstDesc& end, hipStream_t s)
{
    if (ncells == 0 || end.ch_tile0 == 0) return;
    YuvListChroma a{};
    for (int k = 0; k < (semi ? 1 : 2); ++k) { a.src.sp[k] = src[k]; a.src.spitch[k] = spitch[k]; }
    a.src.w = cw; a.src.h = ch;
    a.src.t = tile_tables(cth, ctv);
    a.src.rshift = f ? f->rshift : 0; a.src.mask = f ? f->mask : 0xffu; a.src.lshift = f ? f->lshift : 0;
    a.src.maxv = f ? (float)f->mask : 255.f;
    a.dd = dd; a.n = ncells;
    const dim3 grid(end.ch_tile0);
    switch ((f ? 2 : 0) | (semi ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((k_yuv_list_chroma<1, false>), grid, dim3(kTileThreads), 0, s, a); break;
    case 1: hipLaunchKernelGGL((k_yuv_list_chroma<1, true>), grid, dim3(kTileThreads), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_yuv_list_chroma<2, false>), grid, dim3(kTileThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((k_yuv_list_chroma<2, true>), grid, dim3(kTileThreads), 0, s, a); break;
    }
}

}  // namespace srcnn
