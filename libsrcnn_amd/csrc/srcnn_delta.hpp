// srcnn_delta.hpp -- the host half of the delta call (include/srcnn_amd_delta.h) that needs no device: the tile grid, the two
// span tables that say which source samples a tile depends on, the coalescer that turns the dirty flags into rects, the
// whole-frame rule and the plan of a whole operation (delta_plan).  It needs the contribution-table builder (resample_table.hpp) and the rect geometry (srcnn_rect_source.hpp)
// only -- no HIP -- so tests/host/delta_sanitize.cpp runs it under the CPU sanitizers.  Internal.
//
// The contract.  An output tile grid of tile_w x tile_h output samples covers dw x dh: cols = ceil(dw / tile_w), rows =
// ceil(dh / tile_h), the last column and row may be partial.  Tile (c, r) is DIRTY if and only if some source sample inside
// srcnn_y_path_rect_source(w, h, dw, dh, filter, <tile c,r>) has different 32-bit patterns in the two planes.  That source
// rectangle is xspan[c] x yspan[r]: y_path_rect_source_span treats the axes separately, so one table per axis describes the
// grid, and both ends of a span are non-decreasing in the tile index (the resampler's first tap and last tap are), which is
// what lets the kernel find the tiles of a source sample by bisection.  delta_spans_monotone checks it; the call refuses a
// table that is not.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/srcnn_amd_delta.h"
#include "resample_table.hpp"
#include "srcnn_rect_source.hpp"

namespace srcnn {

constexpr unsigned kDeltaTileDefault = 64;      // the layer kernels' tile width; where the list's cost per rect starts to flatten
constexpr unsigned kDeltaTileMin = 8, kDeltaTileMax = 65535;
// cols and rows each: the kernel holds both span tables and a hit byte per column in LDS, (2 * 4 + 1) * cols + 2 * 4 * rows
// bytes, 34 KB at the limit -- inside the 64 KB a launch gets without asking -- and the flags of a grid are at most 4 MiB
constexpr unsigned kDeltaMaxAxisTiles = 2048;
constexpr unsigned kDeltaListMax = 65536;       // items of a rect list (kRectListMax of srcnn_rect_atlas.hpp)
constexpr unsigned kDeltaHalo = 6;              // a rect's cell: 2 for the 5x5 layer, 4 for the 9x9 layer, on every side

struct DeltaGrid { unsigned tile_w, tile_h, cols, rows; };
struct DeltaSpan { unsigned lo, hi; };          // [lo, hi) of a source axis

// What the delta entry points refuse about the geometry, in the rect call's order, and the grid with the defaults applied.
inline int delta_grid(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h, DeltaGrid& g)
{
    if (w == 0 || h == 0) return fail(SRCNN_E_ARG, "zero dimension (%ux%u)", w, h);
    if (dw == 0 || dh == 0) return fail(SRCNN_E_SCALE, "scaled size %ux%u", dw, dh);
    if (filter < 0 || filter > 4) return fail(SRCNN_E_ARG, "bad filter %d", filter);
    g.tile_w = tile_w ? tile_w : kDeltaTileDefault;
    g.tile_h = tile_h ? tile_h : kDeltaTileDefault;
    if (g.tile_w < kDeltaTileMin || g.tile_w > kDeltaTileMax || g.tile_h < kDeltaTileMin || g.tile_h > kDeltaTileMax)
        return fail(SRCNN_E_ARG, "tile %ux%u: a side is 0 (the default, %u) or %u ... %u", tile_w, tile_h, kDeltaTileDefault, kDeltaTileMin, kDeltaTileMax);
    // the Y path's limits for the frame as one rect
    if (!y_path_fits((unsigned long long)w * h, h, dw, dh, dh))
        return fail(SRCNN_E_UNSUPPORTED, "%ux%u -> %ux%u is beyond the Y path's limits", w, h, dw, dh);
    g.cols = (dw + g.tile_w - 1) / g.tile_w;
    g.rows = (dh + g.tile_h - 1) / g.tile_h;
    if (g.cols > kDeltaMaxAxisTiles || g.rows > kDeltaMaxAxisTiles)
        return fail(SRCNN_E_UNSUPPORTED, "a grid of %u x %u tiles of %ux%u: at most %u a side", g.cols, g.rows, g.tile_w, g.tile_h, kDeltaMaxAxisTiles);
    return SRCNN_OK;
}

// What the *_rects entry points of both delta calls refuse about a grid the caller states: tile sides given, not 0
inline int check_delta_tiles(unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h, unsigned dw, unsigned dh)
{
    if (dw == 0 || dh == 0) return fail(SRCNN_E_SCALE, "scaled size %ux%u", dw, dh);
    if (tile_w < kDeltaTileMin || tile_w > kDeltaTileMax || tile_h < kDeltaTileMin || tile_h > kDeltaTileMax)
        return fail(SRCNN_E_ARG, "tile %ux%u: a side is %u ... %u", tile_w, tile_h, kDeltaTileMin, kDeltaTileMax);
    if (cols != (dw + tile_w - 1) / tile_w || rows != (dh + tile_h - 1) / tile_h)
        return fail(SRCNN_E_ARG, "%u x %u tiles of %ux%u do not cover %ux%u", cols, rows, tile_w, tile_h, dw, dh);
    return SRCNN_OK;
}

// The span table of one axis: entry k is the source range that output tile k = [k * tile, min(dst_len, (k + 1) * tile)) of the
// Y path depends on, exactly as y_path_rect_source_span finds it for one rect -- the tile, +-2 and +-4 cut at the borders, then
// the resampler's taps -- from ONE table of the axis.  first / taps: the axis's contribution table (AxisTable or the device
// cache's host copy); not looked at for an axis that keeps its size, which is copied.
inline void delta_axis_spans(const int* first, const int* taps, unsigned dst_len, unsigned src_len, unsigned tile, std::vector<DeltaSpan>& out)
{
    const unsigned n = (dst_len + tile - 1) / tile;
    out.resize(n);
    for (unsigned k = 0; k < n; ++k) {
        const unsigned a = k * tile, b = std::min(dst_len, a + tile);
        const HaloSpan v = y_path_halo(dst_len, a, b);
        if (dst_len == src_len) out[k] = DeltaSpan{v.ua, v.ub};
        else taps_span(first, taps, src_len, v.ua, v.ub, out[k].lo, out[k].hi);
    }
}

// without a device: the table is built here, once per axis
inline void delta_axis_spans(int filter, unsigned dst_len, unsigned src_len, unsigned tile, std::vector<DeltaSpan>& out)
{
    if (dst_len == src_len) { delta_axis_spans(nullptr, nullptr, dst_len, src_len, tile, out); return; }
    const AxisTable t = build_axis_table(filter, dst_len, src_len);
    delta_axis_spans(t.first.data(), t.taps.data(), dst_len, src_len, tile, out);
}

// both ends non-decreasing, every span inside the axis and not empty: what the kernel's bisection rests on
inline bool delta_spans_monotone(const std::vector<DeltaSpan>& s, unsigned src_len)
{
    for (size_t k = 0; k < s.size(); ++k) {
        if (s[k].lo >= s[k].hi || s[k].hi > src_len) return false;
        if (k && (s[k].lo < s[k - 1].lo || s[k].hi < s[k - 1].hi)) return false;
    }
    return true;
}

// The kernel's table image: xlo[cols], xhi[cols], ylo[rows], yhi[rows]
inline void delta_span_image(const std::vector<DeltaSpan>& xs, const std::vector<DeltaSpan>& ys, unsigned* image)
{
    const size_t cols = xs.size(), rows = ys.size();
    for (size_t c = 0; c < cols; ++c) { image[c] = xs[c].lo; image[cols + c] = xs[c].hi; }
    for (size_t r = 0; r < rows; ++r) { image[2 * cols + r] = ys[r].lo; image[2 * cols + rows + r] = ys[r].hi; }
}
inline size_t delta_span_words(unsigned cols, unsigned rows) { return 2 * ((size_t)cols + rows); }

// ---- the coalescer -----------------------------------------------------------------------------------------------------------
// One deterministic rule.  Tile rows are scanned top to bottom; in each the maximal runs of dirty tiles are taken; a run
// continues the open rect of the previous row when its [c0, c1) is identical, otherwise it opens a new rect.  The rects are
// pairwise disjoint, their union is exactly the dirty tiles clipped to dw x dh, and no clean tile is covered.  `out` gets the
// rects in the order they were OPENED; returns their number.  A flag counts as set when it is not 0.
struct DeltaRect { unsigned x0, y0, rw, rh; };

inline unsigned delta_coalesce(const unsigned char* flags, unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h, unsigned dw, unsigned dh,
                               std::vector<DeltaRect>& out)
{
    struct Open { unsigned c0, c1; size_t rect; };
    std::vector<Open> open, next;            // the runs of the previous tile row, by c0
    out.clear();
    for (unsigned r = 0; r < rows; ++r) {
        const unsigned char* f = flags + (size_t)r * cols;
        const unsigned y0 = r * tile_h, y1 = std::min(dh, y0 + tile_h);
        next.clear();
        size_t o = 0;
        for (unsigned c = 0; c < cols;) {
            if (!f[c]) { ++c; continue; }
            const unsigned c0 = c;
            while (c < cols && f[c]) ++c;
            while (o < open.size() && open[o].c0 < c0) ++o;
            if (o < open.size() && open[o].c0 == c0 && open[o].c1 == c) {
                out[open[o].rect].rh = y1 - out[open[o].rect].y0;
                next.push_back(open[o]);
            } else {
                const unsigned x0 = c0 * tile_w, x1 = std::min(dw, c * tile_w);
                next.push_back(Open{c0, c, out.size()});
                out.push_back(DeltaRect{x0, y0, x1 - x0, y1 - y0});
            }
        }
        open.swap(next);
    }
    return (unsigned)out.size();
}

// The rects as items of the list call that point into the full-size plane d_out (pitch in bytes, not 0; d_out may be NULL: then
// every item's d_out is).  false, and nothing written, when `cap` items do not hold them.
inline bool delta_items(const std::vector<DeltaRect>& rects, float* d_out, size_t pitch, srcnn_rect_item* items, size_t cap)
{
    if (rects.size() > cap) return false;
    const size_t stride = pitch / sizeof(float);
    for (size_t k = 0; k < rects.size(); ++k) {
        const DeltaRect& r = rects[k];
        items[k] = srcnn_rect_item{r.x0, r.y0, r.rw, r.rh, d_out ? d_out + (size_t)r.y0 * stride + r.x0 : nullptr, pitch};
    }
    return true;
}

// ---- the whole-frame rule ------------------------------------------------------------------------------------------------------
inline unsigned long long delta_cell_samples(const std::vector<DeltaRect>& rects)
{
    unsigned long long s = 0;
    for (const DeltaRect& r : rects) s += (unsigned long long)(r.rw + 2 * kDeltaHalo) * (r.rh + 2 * kDeltaHalo);
    return s;
}

// The call repaints the frame as the single item (0, 0, dw, dh) when every tile is dirty, when the list would not hold the
// rects, or when the rects' cells -- what the layers really run over -- reach permille / 1000 of the frame.
inline bool delta_whole_frame(size_t rects, unsigned long long dirty_tiles, unsigned long long tiles, unsigned long long cell_samples,
                              unsigned dw, unsigned dh, long permille)
{
    if (rects == 0) return false;            // nothing changed: nothing is repainted
    if (dirty_tiles == tiles) return true;
    if (rects > kDeltaListMax) return true;
    return cell_samples * 1000ull >= (unsigned long long)permille * ((unsigned long long)dw * dh);
}

// ---- the plan of a whole operation ---------------------------------------------------------------------------------------------
inline unsigned delta_rect_count(size_t n) { return (unsigned)std::min<size_t>(n, 0xffffffffu); }      // srcnn_delta_stats::rects

// From the grid's flags on the host to what is repainted and what the caller is told.  host_flags == NULL: no previous frame --
// every tile counts as dirty and the frame is the one rect.  Otherwise the dirty count and the coalescer, then the whole-frame
// rule, which collapses `rects` to (0, 0, dw, dh); st.rects and st.cell_samples keep what the coalescer gave.  Empty `rects`:
// nothing changed, nothing to repaint.
inline void delta_plan(const unsigned char* host_flags, const DeltaGrid& g, unsigned dw, unsigned dh, long permille, srcnn_delta_stats& st,
                       std::vector<DeltaRect>& rects)
{
    st = srcnn_delta_stats{};
    st.struct_size = (unsigned)sizeof(srcnn_delta_stats);
    st.tiles = g.cols * g.rows;
    if (!host_flags) {
        st.dirty_tiles = st.tiles;
        rects.assign(1, DeltaRect{0, 0, dw, dh});
    } else {
        for (size_t k = 0; k < st.tiles; ++k) st.dirty_tiles += host_flags[k] != 0;
        delta_coalesce(host_flags, g.cols, g.rows, g.tile_w, g.tile_h, dw, dh, rects);
    }
    st.rects = delta_rect_count(rects.size());
    st.cell_samples = delta_cell_samples(rects);
    if (delta_whole_frame(rects.size(), st.dirty_tiles, st.tiles, st.cell_samples, dw, dh, permille)) {
        st.whole_frame = 1;
        rects.assign(1, DeltaRect{0, 0, dw, dh});
    }
}

}  // namespace srcnn
