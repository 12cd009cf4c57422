// srcnn_yuv_packed_rect_list.hip -- the two kernels that join packed YUV frames to the atlas of the rect LIST call
// (include/srcnn_amd_yuv_packed_rect_list.h).  Between them run the list's own launches, unchanged (srcnn_rect_list.hip and the
// layer kernels).
//
//   k_yuvp_list_resample  k_list_resample with an integer fetch: the in-plane part of every cell, resampled by the tile
//                         resampler straight from the caller's packed frame with the luma read rule of k_yuvp_window_y
//                         (srcnn_yuv_packed_window.hip): (float)field * 2^-s.  A fetch loads the ONE dword of the row that
//                         holds the sample's field (luma_field, srcnn_yuv_packed_fields.h), in pieces of the alignment the
//                         frame has: no byte outside the sample's own unit is read, and no float plane of the source exists.
//   k_yuvp_list_merge     one workgroup takes one tile of one item's CHROMA grid (64 x 16 chroma samples, v210: 60 x 16), found by
//                         bisection over ch_tile0 of the destination table (YuvPackedListDstDesc,
//                         srcnn_yuv_packed_rect_atlas.hpp), and runs yuvp_merge_tile (srcnn_yuv_packed_merge_tile.h), the body
//                         of k_yuvp_window_merge, with Y' read from the item's cell of the layer-3 atlas.  A packed row mixes
//                         luma and chroma, so luma and chroma go out in this one launch.  For v210 the last tile of a row of
//                         tiles, by the item's own tile count, owns the groups that only pad the row segment.
//
// Every index is bounded: a tile is cut to its item's chroma columns and rows, the source patch is clamped to the frame
// (tile_patch), source dwords outside [blo, bhi) are not loaded, the cell lies inside the atlas
// (tests/host/rect_list_sanitize.cpp), and a thread stores only bytes of its item's span
// (tests/host/yuv_packed_rect_list_sanitize.cpp recomputes that range off the descriptors).  Every return ahead of a barrier
// depends on the workgroup's item and tile alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_rect_list.h"
#include "srcnn_window_tile.h"
#include "srcnn_yuv.h"
#include "srcnn_yuv_packed_fields.h"
#include "srcnn_yuv_packed_merge_tile.h"
#include "srcnn_yuv_packed_rect_atlas.hpp"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

struct PkListResample {
    const unsigned char* src;                    // the WHOLE packed frame
    size_t spitch;
    unsigned w, h;
    YuvPackedRule f;
    int io;
    TileTables t;                                // the Y tables: horizontal (dw <- w), vertical (dh <- h)
    const ListCellDesc* d;
    unsigned n;
    float* atlas;
    unsigned atlas_w;
};

struct PkListMerge {
    PkMergeSource s;
    const ListCellDesc* d;
    const YuvPackedListDstDesc* dd;              // entry k: the destination of cell k
    unsigned n;
    const float* atlas;                          // the layer-3 result
    unsigned atlas_w;
};

template <int K>
__global__ __launch_bounds__(256) void k_yuvp_list_resample(const PkListResample a)
{
    const int piece = a.io == kIoVec ? kIoDword : a.io;
    list_resample_tile(a.w, a.h, a.t, a.d, a.n, a.atlas, a.atlas_w, [&](size_t sr, size_t sc, float* v) {
        v[0] = (float)luma_field<K>(a.src + sr * a.spitch, sc, a.f, piece) * a.f.down;
    });
}

// the largest k < n with dd[k].ch_tile0 <= b (dd[0].ch_tile0 == 0, and b is below the total)
__device__ __forceinline__ unsigned find_merge_entry(const YuvPackedListDstDesc* __restrict__ dd, unsigned n, unsigned b)
{
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (dd[mid].ch_tile0 <= b) lo = mid; else hi = mid;
    }
    return lo;
}

template <int K>
__global__ __launch_bounds__(256) void k_yuvp_list_merge(const PkListMerge a)
{
    constexpr unsigned kTile = PkItem<K>::TILE;
    const unsigned e = find_merge_entry(a.dd, a.n, blockIdx.x);                          // the same for the whole workgroup
    const YuvPackedListDstDesc o = a.dd[e];
    const ListCellDesc c = a.d[e];
    const unsigned tile = blockIdx.x - o.ch_tile0, tiles_x = (o.ccols + kTile - 1) / kTile;
    const unsigned bx = tile % tiles_x, by = tile / tiles_x;                             // the tile inside the item's chroma grid
    if (bx * kTile >= o.ccols || by * kTileH >= o.rh) return;                            // (never: the prefix sum counts these tiles)
    PkMergeRect r;
    r.dst = reinterpret_cast<unsigned char*>((uintptr_t)o.dst);
    r.dpitch = o.pitch;
    r.y = a.atlas + (size_t)(c.ay + kCellMargin) * a.atlas_w + (c.ax + kCellMargin);     // Y' of the rect's sample (0, 0)
    r.ystride = a.atlas_w;
    r.cx0 = o.cx0; r.gy0 = o.y0; r.row0 = 0;
    r.rw = o.rw; r.ccols = o.ccols; r.rows = o.rh;
    r.groups = o.groups; r.blo = o.blo; r.bhi = o.bhi;
    r.dio = (int)o.io;
    yuvp_merge_tile<K>(a.s, r, bx, by, bx == tiles_x - 1);
}

#define SRCNN_YUVP_LIST_KINDS(X, kind) \
    switch (kind) {                    \
    case kPk422x8: X(kPk422x8); break;   \
    case kPk422x16: X(kPk422x16); break; \
    case kPk444x8: X(kPk444x8); break;   \
    case kPk410: X(kPk410); break;       \
    case kPk444x16: X(kPk444x16); break; \
    default: X(kPkV210); break;          \
    }

}  // namespace

void launch_yuvp_list_resample(const YuvPackedRule& f, const unsigned char* src, size_t spitch, unsigned w, unsigned h, const DevAxisTable& th,
                               const DevAxisTable& tv, const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas,
                               unsigned atlas_w, hipStream_t s)
{
    if (ncells == 0 || end.rs_tile0 == 0) return;
    const PkListResample a{src, spitch, w, h, f, io_of(src, spitch), tile_tables(th, tv), d, ncells, atlas, atlas_w};
    const dim3 grid(end.rs_tile0), b(kTileThreads);
#define SRCNN_YUVP_LIST_RESAMPLE(K) hipLaunchKernelGGL(k_yuvp_list_resample<K>, grid, b, 0, s, a)
    SRCNN_YUVP_LIST_KINDS(SRCNN_YUVP_LIST_RESAMPLE, f.kind)
#undef SRCNN_YUVP_LIST_RESAMPLE
}

void launch_yuvp_list_merge(const YuvPackedRule& f, const unsigned char* src, size_t spitch, unsigned w, unsigned h, const DevAxisTable& cth,
                            const DevAxisTable& ctv, const ListCellDesc* d, const YuvPackedListDstDesc* dd, unsigned ncells,
                            const YuvPackedListDstDesc& end, const float* atlas, unsigned atlas_w, hipStream_t s)
{
    if (ncells == 0 || end.ch_tile0 == 0) return;
    PkListMerge a{};
    a.s.src = src; a.s.spitch = spitch;
    a.s.cw = yuv_packed_chroma_cols(f.kind, w); a.s.h = h;
    a.s.t = tile_tables(cth, ctv);
    a.s.f = f;
    a.s.sio = io_of(src, spitch);
    a.d = d; a.dd = dd; a.n = ncells; a.atlas = atlas; a.atlas_w = atlas_w;
    const dim3 grid(end.ch_tile0), b(kTileThreads);
#define SRCNN_YUVP_LIST_MERGE(K) hipLaunchKernelGGL(k_yuvp_list_merge<K>, grid, b, 0, s, a)
    SRCNN_YUVP_LIST_KINDS(SRCNN_YUVP_LIST_MERGE, f.kind)
#undef SRCNN_YUVP_LIST_MERGE
}

}  // namespace srcnn
