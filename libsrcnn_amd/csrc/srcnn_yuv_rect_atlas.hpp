// srcnn_yuv_rect_atlas.hpp -- what the planar / semi-planar YUV rect LIST call (include/srcnn_amd_yuv_rect_list.h) adds to the
// routing and the descriptor tables of srcnn_rect_atlas.hpp, without a device and without HIP:
// srcnn_yuv_upscale_rect_list_plan and srcnn_yuv_upscale_rect_list_dev run exactly this code, and
// tests/host/yuv_rect_list_sanitize.cpp drives it under the CPU sanitizers.  Internal.
//
// Route.  The Y list's rules for the luma rect (rect_item_batched) and the chroma condition of yuv_rect (srcnn_frames.cpp): the
// CHROMA grid grows in both axes (ccols(dw) > ccols(w), crows(dh) > crows(h): a luma up-scale does not imply it, 4:2:0 with
// w = 3 at 4/3 keeps 2 chroma columns), and the chroma tables on that grid pass window_tile_fits over the item's chroma rect
// (YuvChromaRect).  The cells, the packer and the workspace cap are the Y list's.
//
// Destinations.  The cell table (ListCellDesc) stays as it is; a second table, one YuvListDstDesc per cell of a pass in the
// cell table's order and one closing entry, says where k_yuv_list_luma and k_yuv_list_chroma store: the item's planes and
// pitches, its chroma rect, the prefix sum of 64 x 16 chroma tiles ahead of it (the closing entry: the total), and per plane
// kind whether base and pitch allow one store per thread.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "srcnn_frame_args.hpp"
#include "srcnn_rect_atlas.hpp"

namespace srcnn {

struct YuvRouteInputs {
    RouteInputs y;                                                        // the Y list's inputs, the Y tables in y.th / y.tv
    YuvGeom g;
    TileAxis cth{nullptr, nullptr, 0}, ctv{nullptr, nullptr, 0};          // host copies of the chroma tables (dcw <- cw), (dch <- ch), or NULL
    bool chroma_grows() const { return g.ccols(y.dw) > g.ccols(y.w) && g.crows(y.dh) > g.crows(y.h); }
};

// the chroma half of the decision: what yuv_rect asks before it takes k_yuv_window_chroma
inline bool yuv_chroma_tile_way(const ListRect& r, const YuvRouteInputs& in)
{
    if (!in.chroma_grows()) return false;
    const YuvChromaRect cr(in.g, r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh);
    return window_tile_fits(in.cth, in.ctv, cr.cx0, cr.cx1 - cr.cx0, cr.cy0, cr.cy1 - cr.cy0);
}

inline bool yuv_rect_item_batched(const ListRect& r, const YuvRouteInputs& in) { return rect_item_batched(r, in.y) && yuv_chroma_tile_way(r, in); }

inline RectListRoute route_yuv_rect_list(const ListRect* r, unsigned n, const YuvRouteInputs& in)
{
    return route_rect_list(r, n, in.y, [&](const ListRect& q) { return yuv_chroma_tile_way(q, in); });
}

// The destination of one item of the caller's list, pitches resolved (never 0); semi-planar: plane[2] unused
struct YuvListDst {
    void* plane[3];
    size_t pitch[3];
};

// bytes of the one store a thread makes for its 4 samples of a luma row / its 4 samples (semi-planar: pairs) of a chroma row
inline unsigned yuv_luma_store_bytes(const YuvGeom& g) { return 4u * g.bps; }
inline unsigned yuv_chroma_store_bytes(const YuvGeom& g) { return 4u * g.bps * (g.semi ? 2u : 1u); }

struct YuvListDstDesc {
    unsigned long long plane[3];        // luma sample (x0, y0) first; chroma sample (cx0, cy0) first (semi-planar: plane[1] holds the pairs)
    unsigned long long pitch[3];        // bytes per row
    unsigned cx0, cy0, ccols, crows;    // the chroma rect on the dcw x dch chroma output (YuvChromaRect)
    unsigned ch_tile0;                  // prefix sum of 64 x 16 tiles of the chroma rects ahead of this entry
    unsigned luma_vec;                  // plane[0] and pitch[0] are multiples of yuv_luma_store_bytes
    unsigned chroma_vec;                // every chroma plane's base and pitch are multiples of yuv_chroma_store_bytes
    unsigned reserved;
};
static_assert(sizeof(YuvListDstDesc) == 80, "include/srcnn_amd_yuv_rect_list.h states 80 B per batched item beside the cell's 80");

// The destination table of one pass: pass.count + 1 entries, entry k for cell pass.first + k, entry `count` carrying the chroma
// tile total.  False when that total does not fit 32 bits (never under the Y path's limits -- so it is checked).
inline bool build_yuv_dst_descs(const RectListRoute& route, const AtlasPass& pass, const ListRect* r, const YuvListDst* dst, const YuvGeom& g,
                                std::vector<YuvListDstDesc>& d)
{
    d.assign((size_t)pass.count + 1, YuvListDstDesc{});
    const unsigned ncp = g.semi ? 1u : 2u, lb = yuv_luma_store_bytes(g), cb = yuv_chroma_store_bytes(g);
    unsigned long long tiles = 0;
    for (unsigned k = 0; k < pass.count; ++k) {
        const unsigned item = route.cells[pass.first + k].item;
        const ListRect& q = r[item];
        const YuvListDst& o = dst[item];
        const YuvChromaRect cr(g, q.x0, q.y0, q.x0 + q.rw, q.y0 + q.rh);
        YuvListDstDesc& e = d[k];
        for (unsigned p = 0; p < 1 + ncp; ++p) {
            e.plane[p] = (unsigned long long)reinterpret_cast<uintptr_t>(o.plane[p]);
            e.pitch[p] = o.pitch[p];
        }
        e.cx0 = cr.cx0; e.cy0 = cr.cy0; e.ccols = cr.cx1 - cr.cx0; e.crows = cr.cy1 - cr.cy0;
        e.ch_tile0 = (unsigned)tiles;
        e.luma_vec = (e.plane[0] % lb == 0 && e.pitch[0] % lb == 0) ? 1u : 0u;
        e.chroma_vec = 1;
        for (unsigned p = 1; p < 1 + ncp; ++p)
            if (e.plane[p] % cb || e.pitch[p] % cb) e.chroma_vec = 0;
        tiles += tiles_of(e.ccols, e.crows);
        if (tiles > 0xffffffffull) return false;
    }
    d[pass.count].ch_tile0 = (unsigned)tiles;
    return true;
}

// Bytes of descriptor tables the batched route of a list keeps on the device: a cell entry and a destination entry per batched
// item, and the closing entry of both tables for every atlas
inline unsigned long long yuv_list_desc_bytes(const RectListRoute& route)
{
    return (unsigned long long)(route.cells.size() + route.passes.size()) * (sizeof(ListCellDesc) + sizeof(YuvListDstDesc));
}

}  // namespace srcnn
