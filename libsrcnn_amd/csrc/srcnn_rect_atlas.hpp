// srcnn_rect_atlas.hpp -- routing and packing of the rect LIST call (include/srcnn_amd_rect_list.h), without a device and
// without HIP: srcnn_y_path_rect_list_plan and srcnn_y_path_rect_list_f32_dev run exactly this code, and
// tests/host/rect_list_sanitize.cpp drives it under the CPU sanitizers.  Internal.
//
// Route.  An item is BATCHED when its window can share the layer kernels' launches with the other items' windows: the mode is
// strict, both axes grow, the tile resampler serves its in-plane window (window_tile_fits), and its cell is below the
// single-route threshold and fits the workspace cap alone.  Every other item is SINGLE: y_path_rect, as the single call runs it.
//
// Cell.  A batched item [x0, x0 + rw) x [y0, y0 + rh) owns (rw + 12) x (rh + 12) samples of the atlas; cell sample (i, j) stands
// for plane coordinate (x0 - 6 + i, y0 - 6 + j).  The in-plane part of the cell is resampled, the rest replicated.
//
// Pack.  A shelf packer: the cells in order of decreasing height (ties: wider first, then the lower index) fill rows
// ("shelves") of an atlas from left to right; a cell that does not fit the shelf opens the next one, and a shelf that would
// take 128 B x W x H over the cap opens the next atlas, which runs as another pass out of the same scratch.  The width is at
// least the widest cell left and about the square root of the area left (or of the cap, if that is smaller): of five widths
// from 1x to 1.5x that root the packer keeps the one that fills its atlas best, and the atlas is then cut to the columns in use.
// The order, the widths and the ties are functions of the list alone: the same list gives the same atlases.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "srcnn_window_tile.h"

namespace srcnn {

constexpr unsigned kRectListMax = 65536;             // items of one call
constexpr unsigned kCellMargin = 6;                  // 4 (9x9 layer) + 2 (5x5 layer)
constexpr unsigned long long kAtlasSampleBytes = 128;          // the 32 layer-2 planes: what the workspace cap counts
constexpr unsigned kAtlasMaxW = 0x7fffffu, kAtlasMaxH = 1u << 20;   // the Y path's limits hold for an atlas as for a frame

struct ListRect { unsigned x0, y0, rw, rh; };        // inside dw x dh, not empty (the entry points have checked)

struct AtlasCell {
    unsigned item;          // index in the caller's list
    unsigned pass;          // the atlas it lies in
    unsigned ax, ay;        // the cell's first sample in that atlas
    unsigned cw, ch;        // rw + 12, rh + 12
};
struct AtlasPass {
    unsigned W, H;          // the atlas: a frame of its own for the layer kernels
    unsigned first, count;  // its cells: [first, first + count) of RectListRoute::cells
};
struct RectListRoute {
    std::vector<unsigned> single;       // items of the single route, in list order
    std::vector<AtlasCell> cells;       // items of the batched route, pass by pass
    std::vector<AtlasPass> passes;
    unsigned long long cell_samples = 0, atlas_samples = 0;
};

struct RouteInputs {
    unsigned w = 0, h = 0, dw = 0, dh = 0;
    bool strict = true;                 // SRCNN_MODE_STRICT
    bool unfused = false;               // SRCNN_RECT_LIST_UNFUSED, or a stream in a foreign capture
    unsigned long long cap_bytes = 0;   // srcnn_set_workspace_limit
    unsigned long long single_samples = 0;      // SRCNN_RECT_LIST_SINGLE_SAMPLES
    TileAxis th{nullptr, nullptr, 0}, tv{nullptr, nullptr, 0};      // host copies of the tables (dw <- w), (dh <- h), or NULL
};

// What a cell is on the plane, per axis: the first in-plane coordinate, how many, and where they start in the cell.
struct CellAxis {
    unsigned p0, n, off;
    CellAxis(unsigned a, unsigned len, unsigned dst) : p0(a >= kCellMargin ? a - kCellMargin : 0), n(std::min(dst, a + len + kCellMargin) - p0), off(p0 - a + kCellMargin) {}
};

inline bool rect_item_batched(const ListRect& r, const RouteInputs& in)
{
    if (!in.strict || in.unfused || in.dw <= in.w || in.dh <= in.h) return false;
    const unsigned long long cw = (unsigned long long)r.rw + 2 * kCellMargin, ch = (unsigned long long)r.rh + 2 * kCellMargin;
    if (cw > kAtlasMaxW || ch > kAtlasMaxH) return false;
    const unsigned long long area = cw * ch;
    if (area >= in.single_samples || area > in.cap_bytes / kAtlasSampleBytes) return false;
    const CellAxis cx(r.x0, r.rw, in.dw), cy(r.y0, r.rh, in.dh);
    return window_tile_fits(in.th, in.tv, cx.p0, cx.n, cy.p0, cy.n);
}

namespace atlas_detail {

inline unsigned long long isqrt_ceil(unsigned long long v)
{
    unsigned long long r = 0;
    for (unsigned long long bit = 1ull << 31; bit; bit >>= 1)
        if ((r + bit) * (r + bit) <= v) r += bit;
    return r * r == v ? r : r + 1;
}

struct Trial { unsigned count = 0, W = 0, H = 0; unsigned long long cells = 0; };

// Shelves of width `width` from cells[first ...] on, in order; place == true writes the positions.  Stops at the first cell that
// needs a shelf the cap (in samples) or the limits refuse; the first cell of an atlas is always taken (the router has checked it
// alone), in an atlas as narrow as the cap asks.
inline Trial shelve(std::vector<AtlasCell>& cells, size_t first, unsigned long long width, unsigned long long cap, bool place, unsigned pass)
{
    Trial t;
    const AtlasCell& head = cells[first];
    if (width * head.ch > cap) width = std::max<unsigned long long>(head.cw, cap / head.ch);
    width = std::min<unsigned long long>(std::max<unsigned long long>(width, head.cw), kAtlasMaxW);
    unsigned long long x = 0, y = 0, shelf = 0, used = 0;
    for (size_t k = first; k < cells.size(); ++k) {
        AtlasCell& c = cells[k];
        if (c.cw > width) break;
        if (shelf == 0 || x + c.cw > width) {              // a new shelf (heights only fall: the first cell sets it)
            const unsigned long long ny = y + shelf;
            if (k != first && (width * (ny + c.ch) > cap || ny + c.ch > kAtlasMaxH)) break;
            y = ny; x = 0; shelf = c.ch;
        }
        if (place) { c.ax = (unsigned)x; c.ay = (unsigned)y; c.pass = pass; }
        x += c.cw;
        used = std::max(used, x);
        t.cells += (unsigned long long)c.cw * c.ch;
        ++t.count;
    }
    t.W = (unsigned)used;
    t.H = (unsigned)(y + shelf);
    return t;
}

}  // namespace atlas_detail

// Packs route.cells (item, cw, ch set) into passes under the cap; fills ax, ay, pass, route.passes and the two sums.
inline void pack_rect_cells(RectListRoute& route, unsigned long long cap_bytes)
{
    using namespace atlas_detail;
    std::vector<AtlasCell>& cells = route.cells;
    std::sort(cells.begin(), cells.end(), [](const AtlasCell& a, const AtlasCell& b) {
        if (a.ch != b.ch) return a.ch > b.ch;
        if (a.cw != b.cw) return a.cw > b.cw;
        return a.item < b.item;
    });
    const unsigned long long cap = cap_bytes / kAtlasSampleBytes;
    // area and widest cell of cells[k ...]
    std::vector<unsigned long long> area_from(cells.size() + 1, 0);
    std::vector<unsigned> widest_from(cells.size() + 1, 0);
    for (size_t k = cells.size(); k-- > 0;) {
        area_from[k] = area_from[k + 1] + (unsigned long long)cells[k].cw * cells[k].ch;
        widest_from[k] = std::max(widest_from[k + 1], cells[k].cw);
    }
    route.cell_samples = area_from[0];
    route.atlas_samples = 0;
    route.passes.clear();
    for (size_t first = 0; first < cells.size();) {
        const unsigned long long root = isqrt_ceil(std::min(area_from[first], cap));
        unsigned long long best_w = 0;
        Trial best;
        for (unsigned k = 0; k <= 4; ++k) {
            const unsigned long long width = std::max<unsigned long long>(widest_from[first], root + root * k / 8);
            const Trial t = shelve(cells, first, width, cap, false, 0);
            // better fill = cells / (W * H), compared without division; ties keep the narrower trial
            if (best.count == 0 || t.cells * ((unsigned long long)best.W * best.H) > best.cells * ((unsigned long long)t.W * t.H)) { best = t; best_w = width; }
        }
        const unsigned pass = (unsigned)route.passes.size();
        const Trial t = shelve(cells, first, best_w, cap, true, pass);
        route.passes.push_back(AtlasPass{t.W, t.H, (unsigned)first, t.count});
        route.atlas_samples += (unsigned long long)t.W * t.H;
        first += t.count;
    }
}

// The whole decision for a list: who goes which way, and where the batched cells lie.  extra(rect): one more condition on a
// batched item (the colour shells of srcnn_rgb_rect_atlas.hpp, srcnn_yuv_rect_atlas.hpp and srcnn_yuv_packed_rect_atlas.hpp)
template <class Extra>
inline RectListRoute route_rect_list(const ListRect* r, unsigned n, const RouteInputs& in, Extra extra)
{
    RectListRoute route;
    for (unsigned k = 0; k < n; ++k) {
        if (rect_item_batched(r[k], in) && extra(r[k])) route.cells.push_back(AtlasCell{k, 0, 0, 0, r[k].rw + 2 * kCellMargin, r[k].rh + 2 * kCellMargin});
        else route.single.push_back(k);
    }
    pack_rect_cells(route, in.cap_bytes);
    return route;
}
inline RectListRoute route_rect_list(const ListRect* r, unsigned n, const RouteInputs& in)
{
    return route_rect_list(r, n, in, [](const ListRect&) { return true; });
}

// ---- what the kernels of srcnn_rect_list.hip read: one descriptor per cell of a pass, and one closing entry that holds the totals ----
struct ListCellDesc {
    unsigned ax, ay, cw, ch;            // the cell in the atlas
    unsigned px, py, iw, ih;            // its in-plane part on the dw x dh plane ...
    unsigned ox, oy;                    // ... and where that part starts inside the cell
    unsigned rw, rh;                    // the rect (at (6, 6) of the cell)
    unsigned rs_tile0, rep_tile0, sc_tile0;      // prefix sums of 64 x 16 tiles: in-plane part / whole cell if it has an out-of-plane part / rect
    unsigned out_vec;                   // d_out and its pitch allow 16-byte stores
    unsigned long long out;             // d_out
    unsigned long long out_stride;      // floats per row of d_out
};

inline unsigned tiles_of(unsigned wd, unsigned ht) { return ((wd + kTileW - 1) / kTileW) * ((ht + kTileH - 1) / kTileH); }

struct ListOut { void* d_out; size_t out_stride; };      // per item of the caller's list; stride in floats

// The descriptor table of one pass: count + 1 entries, entry `count` carrying the three tile totals.  False when a total does
// not fit 32 bits (never under the limits above: an atlas has at most 2^43 samples, i.e. 2^33 tiles -- so it is checked).
inline bool build_cell_descs(const RectListRoute& route, const AtlasPass& pass, const ListRect* r, const ListOut* out, unsigned dw, unsigned dh,
                             std::vector<ListCellDesc>& d)
{
    d.assign((size_t)pass.count + 1, ListCellDesc{});
    unsigned long long rs = 0, rep = 0, sc = 0;
    for (unsigned k = 0; k < pass.count; ++k) {
        const AtlasCell& c = route.cells[pass.first + k];
        const ListRect& q = r[c.item];
        const CellAxis cx(q.x0, q.rw, dw), cy(q.y0, q.rh, dh);
        ListCellDesc& e = d[k];
        e.ax = c.ax; e.ay = c.ay; e.cw = c.cw; e.ch = c.ch;
        e.px = cx.p0; e.py = cy.p0; e.iw = cx.n; e.ih = cy.n; e.ox = cx.off; e.oy = cy.off;
        e.rw = q.rw; e.rh = q.rh;
        e.rs_tile0 = (unsigned)rs; e.rep_tile0 = (unsigned)rep; e.sc_tile0 = (unsigned)sc;
        if (out) {
            e.out = (unsigned long long)reinterpret_cast<uintptr_t>(out[c.item].d_out);
            e.out_stride = out[c.item].out_stride;
            e.out_vec = (e.out % 16 == 0 && (e.out_stride % 4 == 0 || q.rh == 1)) ? 1u : 0u;
        }
        rs += tiles_of(cx.n, cy.n);
        if (cx.n != c.cw || cy.n != c.ch) rep += tiles_of(c.cw, c.ch);
        sc += tiles_of(q.rw, q.rh);
        if (rs > 0xffffffffull || rep > 0xffffffffull || sc > 0xffffffffull) return false;
    }
    ListCellDesc& end = d[pass.count];
    end.rs_tile0 = (unsigned)rs; end.rep_tile0 = (unsigned)rep; end.sc_tile0 = (unsigned)sc;
    return true;
}

// ---- where the tables of a batched list lie, in the staging slot on the host and in Workspace::list on the device alike ----
// The cell tables of every pass (count + 1 entries each), then -- for a list that has a second table -- the destination tables
// of every pass: count entries each, and a closing one where the surface's kernels want a total (dst_closing == 1).  The passes
// of a route follow each other in `cells`, so the first entry of pass k is its `first` plus the closing entries ahead of it.
struct ListTableLayout {
    size_t dst_entry_bytes;             // 0: no destination table (the Y list)
    unsigned dst_closing;               // 0 / 1 closing entries per pass of the destination table
    size_t dst_offset;                  // bytes of the cell tables = where the destination tables begin (80 is a multiple of 8)
    size_t bytes;                       // both tables
    ListTableLayout(const RectListRoute& route, size_t dst_entry_bytes_, unsigned dst_closing_)
        : dst_entry_bytes(dst_entry_bytes_), dst_closing(dst_closing_), dst_offset((route.cells.size() + route.passes.size()) * sizeof(ListCellDesc)),
          bytes(dst_offset + (dst_entry_bytes_ ? (route.cells.size() + route.passes.size() * dst_closing_) * dst_entry_bytes_ : 0))
    {
    }
    size_t cell_first(const RectListRoute& route, size_t k) const { return route.passes[k].first + k; }
    size_t dst_first(const RectListRoute& route, size_t k) const { return route.passes[k].first + k * dst_closing; }
    // the tables of pass k in a buffer that begins at `base`
    ListCellDesc* cells(unsigned char* base, const RectListRoute& route, size_t k) const { return reinterpret_cast<ListCellDesc*>(base) + cell_first(route, k); }
    template <class Dst>
    Dst* dsts(unsigned char* base, const RectListRoute& route, size_t k) const { return reinterpret_cast<Dst*>(base + dst_offset) + dst_first(route, k); }
};

}  // namespace srcnn
