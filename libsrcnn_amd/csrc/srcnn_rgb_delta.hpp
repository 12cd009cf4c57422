// srcnn_rgb_delta.hpp -- what the RGB(A) delta call (include/srcnn_amd_rgb_delta.h) adds to the host half of srcnn_delta.hpp: the
// span tables of an RGB(A) tile grid and the rects as items of the RGB(A) rect list call.  The grid, the coalescer, the cell
// count and the whole-frame rule are srcnn_delta.hpp's, used as they are.  No HIP, so tests/host/rgb_delta_sanitize.cpp runs it
// under the CPU sanitizers.  Internal.
//
// The contract.  Tile (c, r) is DIRTY if and only if some pixel inside srcnn_rgb_rect_source(w, h, multiply, filter, <tile c,r>)
// has a differing byte.  That rectangle is the union of the Y path's source rectangle of the tile (halo of 6, then the taps of
// `filter`) and of the taps chroma_filter(filter) gives for the tile itself; both parts treat the axes separately, so the union
// does too: one table per axis, entry k = [min of the two lower ends, max of the two upper ends).  Neither part is assumed to
// hold the other.  Both ends of both parts are non-decreasing in k, so the ends of the union are; delta_spans_monotone stays the
// gate.  All planes of an RGB(A) image share the pixel grid, so one pair of tables serves them all.
#pragma once
#include "../../include/srcnn_amd_rgb_rect_list.h"
#include "srcnn_delta.hpp"
#include "srcnn_rgb_rect_atlas.hpp"

namespace srcnn {

// The span table of one axis of an RGB(A) grid.  yfirst / ytaps: the axis's contribution table for `filter`, cfirst / ctaps:
// for chroma_filter(filter) (AxisTable or the device cache's host copy); neither is looked at for an axis that keeps its size,
// which is copied on both parts.
inline void rgb_delta_axis_spans(const int* yfirst, const int* ytaps, const int* cfirst, const int* ctaps, unsigned dst_len, unsigned src_len,
                                 unsigned tile, std::vector<DeltaSpan>& out)
{
    delta_axis_spans(yfirst, ytaps, dst_len, src_len, tile, out);         // the Y path's part
    for (unsigned k = 0; k < out.size(); ++k) {
        const unsigned a = k * tile, b = std::min(dst_len, a + tile);
        unsigned lo = a, hi = b;
        if (dst_len != src_len) taps_span(cfirst, ctaps, src_len, a, b, lo, hi);
        out[k].lo = std::min(out[k].lo, lo);
        out[k].hi = std::max(out[k].hi, hi);
    }
}

// without a device: the two tables are built here, once per axis
inline void rgb_delta_axis_spans(int filter, unsigned dst_len, unsigned src_len, unsigned tile, std::vector<DeltaSpan>& out)
{
    if (dst_len == src_len) { rgb_delta_axis_spans(nullptr, nullptr, nullptr, nullptr, dst_len, src_len, tile, out); return; }
    const AxisTable y = build_axis_table(filter, dst_len, src_len), c = build_axis_table(chroma_filter(filter), dst_len, src_len);
    rgb_delta_axis_spans(y.first.data(), y.taps.data(), c.first.data(), c.taps.data(), dst_len, src_len, tile, out);
}

// The full-size destination image the items point into: pitches resolved (never 0); plane[p] == NULL for every p: the items'
// destinations are NULL; conv == NULL: no truncated Y' plane
using RgbDeltaDst = RgbListDst;

// The rects as items of the RGB(A) list call: an item's dst[p] (and dst_conv) is the address of pixel (x0, y0) of the full-size
// image, with the image's pitch.  false, and nothing written, when `cap` items do not hold them.
inline bool rgb_delta_items(const std::vector<DeltaRect>& rects, const RgbListLayout& lay, const RgbDeltaDst& d, srcnn_rgb_rect_item* items, size_t cap)
{
    if (rects.size() > cap) return false;
    const size_t bpp = lay.row_bytes(1);                                   // bytes of a pixel in one plane's row
    for (size_t k = 0; k < rects.size(); ++k) {
        const DeltaRect& r = rects[k];
        srcnn_rgb_rect_item it{};
        it.x0 = r.x0; it.y0 = r.y0; it.rw = r.rw; it.rh = r.rh;
        for (unsigned p = 0; p < lay.planes(); ++p) {
            it.dst[p] = d.plane[p] ? static_cast<unsigned char*>(d.plane[p]) + (size_t)r.y0 * d.pitch[p] + (size_t)r.x0 * bpp : nullptr;
            it.dst_pitch[p] = d.pitch[p];
        }
        it.dst_conv = d.conv ? static_cast<unsigned char*>(d.conv) + (size_t)r.y0 * d.conv_pitch + (size_t)r.x0 * lay.bps : nullptr;
        it.dst_conv_pitch = d.conv ? d.conv_pitch : 0;
        items[k] = it;
    }
    return true;
}

}  // namespace srcnn
