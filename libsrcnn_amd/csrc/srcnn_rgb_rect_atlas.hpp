// srcnn_rgb_rect_atlas.hpp -- what the RGB(A) rect LIST call (include/srcnn_amd_rgb_rect_list.h) adds to the routing and the
// descriptor tables of srcnn_rect_atlas.hpp, without a device and without HIP: srcnn_rgb_upscale_rect_list_plan and
// srcnn_rgb_upscale_rect_list_dev run exactly this code, and tests/host/rgb_rect_list_sanitize.cpp drives it under the CPU
// sanitizers.  Internal.
//
// Route.  The Y list's rules (rect_item_batched) and one more: the merge kernel resamples Cb, Cr (and A) of the rect itself,
// [x0, x0 + rw) x [y0, y0 + rh), tile by tile with the chroma tables, so those must pass window_tile_fits for the rect.  The
// cells, the packer and the workspace cap are the Y list's.
//
// Destinations.  The cell table (ListCellDesc) stays as it is; a second table, one ListDstDesc per cell of a pass and in the
// cell table's order, says where k_rgb_list_merge stores the rect of that cell: the item's planes, pitches, dst_conv, and
// whether its bases and pitches allow 4-byte stores.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "srcnn_rect_atlas.hpp"

namespace srcnn {

struct RgbRouteInputs {
    RouteInputs y;                                                        // the Y list's inputs, the Y tables in y.th / y.tv
    TileAxis cth{nullptr, nullptr, 0}, ctv{nullptr, nullptr, 0};          // host copies of the chroma tables (dw <- w), (dh <- h), or NULL
};

inline bool rgb_rect_item_batched(const ListRect& r, const RgbRouteInputs& in)
{
    return rect_item_batched(r, in.y) && window_tile_fits(in.cth, in.ctv, r.x0, r.rw, r.y0, r.rh);
}

inline RectListRoute route_rgb_rect_list(const ListRect* r, unsigned n, const RgbRouteInputs& in)
{
    return route_rect_list(r, n, in.y, [&](const ListRect& q) { return window_tile_fits(in.cth, in.ctv, q.x0, q.rw, q.y0, q.rh); });
}

// What a format comes down to for the destination table: bytes per sample, channels, one plane per channel or one for all
struct RgbListLayout {
    unsigned bps, ch;
    bool planar;
    unsigned planes() const { return planar ? ch : 1u; }
    size_t row_bytes(unsigned rw) const { return (size_t)bps * (planar ? 1u : ch) * rw; }
};

// The destination of one item of the caller's list, pitches resolved (never 0); conv == NULL: no truncated Y' plane
struct RgbListDst {
    void* plane[4];
    size_t pitch[4];
    void* conv;
    size_t conv_pitch;
};

struct ListDstDesc {
    unsigned long long plane[4];        // the item's planes: pixel (x0, y0) first (interleaved: plane[0] only)
    unsigned long long pitch[4];        // bytes per row
    unsigned long long conv;            // dst_conv, or 0
    unsigned long long conv_pitch;
    unsigned int_vec;                   // every plane's base and pitch are multiples of 4: 4 pixels go out in 4-byte words
    unsigned conv_vec;                  // the same for dst_conv
};
static_assert(sizeof(ListDstDesc) == 88, "include/srcnn_amd_rgb_rect_list.h states 88 B per batched item beside the cell's 80");

// The destination table of one pass: pass.count entries, entry k for cell pass.first + k
inline void build_dst_descs(const RectListRoute& route, const AtlasPass& pass, const RgbListDst* dst, const RgbListLayout& f, std::vector<ListDstDesc>& d)
{
    d.assign((size_t)pass.count, ListDstDesc{});
    for (unsigned k = 0; k < pass.count; ++k) {
        const RgbListDst& q = dst[route.cells[pass.first + k].item];
        ListDstDesc& e = d[k];
        e.int_vec = 1;
        for (unsigned p = 0; p < f.planes(); ++p) {
            e.plane[p] = (unsigned long long)reinterpret_cast<uintptr_t>(q.plane[p]);
            e.pitch[p] = q.pitch[p];
            if (e.plane[p] % 4 || e.pitch[p] % 4) e.int_vec = 0;
        }
        e.conv = (unsigned long long)reinterpret_cast<uintptr_t>(q.conv);
        e.conv_pitch = q.conv ? q.conv_pitch : 0;
        e.conv_vec = (q.conv && e.conv % 4 == 0 && e.conv_pitch % 4 == 0) ? 1u : 0u;
    }
}

// Bytes of descriptor tables the batched route of a list keeps on the device: a cell entry and a destination entry per batched
// item, and the closing cell entry of every atlas
inline unsigned long long rgb_list_desc_bytes(const RectListRoute& route)
{
    return (unsigned long long)(route.cells.size() + route.passes.size()) * sizeof(ListCellDesc) + (unsigned long long)route.cells.size() * sizeof(ListDstDesc);
}

}  // namespace srcnn
