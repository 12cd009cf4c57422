// srcnn_yuv_packed_rect_atlas.hpp -- what the packed YUV rect LIST call (include/srcnn_amd_yuv_packed_rect_list.h) adds to the
// routing and the descriptor tables of srcnn_rect_atlas.hpp, without a device and without HIP:
// srcnn_yuv_packed_upscale_rect_list_plan and srcnn_yuv_packed_upscale_rect_list_dev run exactly this code, and
// tests/host/yuv_packed_rect_list_sanitize.cpp drives it under the CPU sanitizers.  Internal.
//
// Route.  The Y list's rules for the luma rect (rect_item_batched) and the chroma condition of yuv_packed_rect
// (srcnn_frames.cpp): the CHROMA grid grows in both axes (ccols(dw) > ccols(w), dh > h: a luma up-scale does not imply the
// first, a 4:2:2 format with w = 1 at 2x keeps 1 chroma column), and the chroma tables on that grid pass yuvp_window_fits -- the
// tile predicate at the width k_yuvp_list_merge really uses, 60 columns for v210 -- over the item's chroma columns and all rh
// rows.  The cells, the packer and the workspace cap are the Y list's.
//
// Destinations.  The cell table (ListCellDesc) stays as it is; a second table, one YuvPackedListDstDesc per cell of a pass in the
// cell table's order and one closing entry, says what k_yuvp_list_merge stores and where: the item's first byte and pitch, its
// chroma columns, rows and luma width, v210's groups per row segment, the bytes of a source row its chroma taps may read, the
// store path, and the prefix sum of chroma tiles (64 x 16, v210: 60 x 16) ahead of it (the closing entry: the total).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "srcnn_frame_args.hpp"
#include "srcnn_rect_atlas.hpp"
#include "srcnn_rect_source.hpp"

namespace srcnn {

struct YuvPackedRouteInputs {
    RouteInputs y;                                                        // the Y list's inputs, the Y tables in y.th / y.tv
    int kind = kPk422x8;
    TileAxis cth{nullptr, nullptr, 0}, ctv{nullptr, nullptr, 0};          // host copies of the chroma tables (dcw <- cw), (dh <- h), or NULL
    bool chroma_grows() const { return yuv_packed_chroma_cols(kind, y.dw) > yuv_packed_chroma_cols(kind, y.w) && y.dh > y.h; }
};

// the chroma half of the decision: what yuv_packed_rect asks before it takes k_yuvp_window_merge, over all rows of the rect
inline bool yuvp_chroma_tile_way(const ListRect& r, const YuvPackedRouteInputs& in)
{
    if (!in.chroma_grows()) return false;
    const YuvPackedChromaCols cc(in.kind, r.x0, r.x0 + r.rw);
    return yuvp_window_fits(in.kind, in.cth, in.ctv, cc.cx0, cc.cx1 - cc.cx0, r.y0, r.rh);
}

inline bool yuv_packed_rect_item_batched(const ListRect& r, const YuvPackedRouteInputs& in)
{
    return rect_item_batched(r, in.y) && yuvp_chroma_tile_way(r, in);
}

inline RectListRoute route_yuv_packed_rect_list(const ListRect* r, unsigned n, const YuvPackedRouteInputs& in)
{
    return route_rect_list(r, n, in.y, [&](const ListRect& q) { return yuvp_chroma_tile_way(q, in); });
}

// The destination of one item of the caller's list, the pitch resolved (never 0)
struct YuvPackedListDst {
    void* dst;
    size_t pitch;
};

struct YuvPackedListDstDesc {
    unsigned long long dst;             // the byte at `off` of row y0 (yuv_packed_span of the rect)
    unsigned long long pitch;           // bytes per row
    unsigned cx0, y0;                   // the rect's first chroma column on the dcw-wide chroma output, its first output row
    unsigned ccols, rw, rh;             // chroma columns, luma columns, rows
    unsigned groups;                    // 16-byte groups of a row segment (v210: the padding groups at the right border included)
    unsigned blo, bhi;                  // bytes of a source row the chroma taps of the rect's columns may read
    unsigned io;                        // io_of(dst, pitch): kIoVec where base and pitch are multiples of 16
    unsigned ch_tile0;                  // prefix sum of yuv_packed_tile_cols x 16 tiles of the chroma grids ahead of this entry
    unsigned reserved[2];
};
static_assert(sizeof(YuvPackedListDstDesc) == 64, "include/srcnn_amd_yuv_packed_rect_list.h states 64 B per batched item beside the cell's 80");

inline unsigned long long yuvp_tiles_of(int kind, unsigned ccols, unsigned rows)
{
    const unsigned tile = yuv_packed_tile_cols(kind);
    return (unsigned long long)((ccols + tile - 1) / tile) * ((rows + kTileH - 1) / kTileH);
}

// Bytes [blo, bhi) of a row of the w-pixel source that the taps of chroma output columns [cx0, cx0 + ccols) read, widened to the
// unit: the range launch_yuvp_window_merge (srcnn_yuv_packed_window.hip) allows its kernel.  cth: the host copy of (dcw <- cw).
inline void yuvp_tap_bytes(int kind, unsigned w, const TileAxis& cth, unsigned cx0, unsigned ccols, unsigned& blo, unsigned& bhi)
{
    int lo = 0x7fffffff, hi = 0;
    for (unsigned x = cx0; x < cx0 + ccols; ++x) { lo = std::min(lo, cth.first[x]); hi = std::max(hi, cth.first[x] + cth.taps[x]); }
    const unsigned step = yuv_packed_chroma_step(kind);
    yuv_packed_unit_span(kind, w, (unsigned)std::max(lo, 0) * step, std::min((unsigned)hi * step, w), blo, bhi);
}

// The destination table of one pass: pass.count + 1 entries, entry k for cell pass.first + k, entry `count` carrying the chroma
// tile total.  w, dw: the frame's and the output's width; cth: the host copy of the horizontal chroma table (the router has
// asked yuvp_window_fits, so it is there).  False when the total does not fit 32 bits (never under the Y path's limits -- so it
// is checked).
inline bool build_yuv_packed_dst_descs(const RectListRoute& route, const AtlasPass& pass, const ListRect* r, const YuvPackedListDst* dst, int kind,
                                       unsigned w, unsigned dw, const TileAxis& cth, std::vector<YuvPackedListDstDesc>& d)
{
    d.assign((size_t)pass.count + 1, YuvPackedListDstDesc{});
    unsigned long long tiles = 0;
    for (unsigned k = 0; k < pass.count; ++k) {
        const unsigned item = route.cells[pass.first + k].item;
        const ListRect& q = r[item];
        const YuvPackedListDst& o = dst[item];
        const YuvPackedChromaCols cc(kind, q.x0, q.x0 + q.rw);
        size_t off = 0, n = 0;
        yuv_packed_span(kind, dw, q.x0, q.rw, off, n);
        YuvPackedListDstDesc& e = d[k];
        e.dst = (unsigned long long)reinterpret_cast<uintptr_t>(o.dst);
        e.pitch = o.pitch;
        e.cx0 = cc.cx0; e.y0 = q.y0;
        e.ccols = cc.cx1 - cc.cx0; e.rw = q.rw; e.rh = q.rh;
        e.groups = (unsigned)(n / 16);
        yuvp_tap_bytes(kind, w, cth, e.cx0, e.ccols, e.blo, e.bhi);
        e.io = (unsigned)io_of(o.dst, o.pitch);
        e.ch_tile0 = (unsigned)tiles;
        tiles += yuvp_tiles_of(kind, e.ccols, e.rh);
        if (tiles > 0xffffffffull) return false;
    }
    d[pass.count].ch_tile0 = (unsigned)tiles;
    return true;
}

// Bytes of descriptor tables the batched route of a list keeps on the device: a cell entry and a destination entry per batched
// item, and the closing entry of both tables for every atlas
inline unsigned long long yuv_packed_list_desc_bytes(const RectListRoute& route)
{
    return (unsigned long long)(route.cells.size() + route.passes.size()) * (sizeof(ListCellDesc) + sizeof(YuvPackedListDstDesc));
}

}  // namespace srcnn
