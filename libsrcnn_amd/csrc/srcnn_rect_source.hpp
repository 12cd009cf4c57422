// srcnn_rect_source.hpp -- which part of a source plane a rect of the output depends on, without a device: the geometry behind
// srcnn_y_path_rect_source, srcnn_rgb_rect_source, srcnn_yuv_rect_source and srcnn_yuv_packed_rect_source (with
// srcnn_yuv_packed_span_bytes).  It needs the contribution-table builder
// (resample_table.hpp) and the argument checks (srcnn_frame_args.hpp) only -- no HIP -- so tests/host/yuv_rect_sanitize.cpp
// runs it under the CPU sanitizers.  Internal.
#pragma once
#include <algorithm>

#include "resample_table.hpp"
#include "srcnn_frame_args.hpp"
#include "srcnn_window_tile.h"
#include "srcnn_y_path_geom.hpp"

namespace srcnn {

// [lo,hi) of the source axis that destination indices [a,b) of the resampled axis read: the taps of the range, read off the
// table; an axis that keeps its size is copied
inline void axis_source_span(int filter, unsigned dst_len, unsigned src_len, unsigned a, unsigned b, unsigned& lo, unsigned& hi)
{
    if (dst_len == src_len) { lo = a; hi = b; return; }
    const AxisTable t = build_axis_table(filter, dst_len, src_len);
    taps_span(t.first.data(), t.taps.data(), src_len, a, b, lo, hi);
}

// [lx,hx) x [ly,hy) of the w x h plane that samples [x0,x1) x [y0,y1) of the Y path's dw x dh output depend on: the rect, +-2
// (layer 3) and +-4 (layer 1) cut at the borders, then the resampler's taps.  The rect lies inside the output.
inline void y_path_rect_source_span(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned x0, unsigned y0, unsigned x1,
                                    unsigned y1, unsigned& lx, unsigned& hx, unsigned& ly, unsigned& hy)
{
    const HaloSpan vx = y_path_halo(dw, x0, x1), vy = y_path_halo(dh, y0, y1);
    axis_source_span(filter, dw, w, vx.ua, vx.ub, lx, hx);
    axis_source_span(filter, dh, h, vy.ua, vy.ub, ly, hy);
}

// chroma and alpha planes: nearest stays nearest, everything else is bilinear (as J.cfilter of srcnn_process_u8)
inline int chroma_filter(int filter) { return filter == SRCNN_FILTER_NEAREST ? SRCNN_FILTER_NEAREST : SRCNN_FILTER_BILINEAR; }

// srcnn_yuv_rect_source (include/srcnn_amd_yuv_rect.h)
inline int yuv_rect_source(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter, unsigned x0, unsigned y0,
                           unsigned rw, unsigned rh, int plane, unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh)
{
    YuvGeom g;
    unsigned dw = 0, dh = 0, lx = 0, ly = 0, hx = 0, hy = 0;
    int rc;
    if ((rc = yuv_geom_from_format(fmt, g))) return rc;
    if (plane < 0 || plane > 2) return fail(SRCNN_E_ARG, "plane %d", plane);
    if (rw == 0 || rh == 0) return fail(SRCNN_E_ARG, "empty rect %ux%u", rw, rh);
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;       // (its limits include those of srcnn_y_path_rect_source)
    if ((rc = check_rect_inside(dw, dh, x0, y0, rw, rh))) return rc;
    if ((rc = check_yuv_rect_origin(g, x0, y0))) return rc;
    if (plane == 0) {
        y_path_rect_source_span(w, h, dw, dh, filter, x0, y0, x0 + rw, y0 + rh, lx, hx, ly, hy);
    } else if (!(g.semi && plane == 2)) {
        const YuvChromaRect cr(g, x0, y0, x0 + rw, y0 + rh);
        const int cfilter = chroma_filter(filter);
        axis_source_span(cfilter, g.ccols(dw), g.ccols(w), cr.cx0, cr.cx1, lx, hx);
        axis_source_span(cfilter, g.crows(dh), g.crows(h), cr.cy0, cr.cy1, ly, hy);
    }
    if (sx0) *sx0 = lx;
    if (sy0) *sy0 = ly;
    if (sw) *sw = hx - lx;
    if (sh) *sh = hy - ly;
    return SRCNN_OK;
}

// ---- packed frames (include/srcnn_amd_yuv_packed_rect.h) ----

// srcnn_yuv_packed_span_bytes
inline int yuv_packed_span_bytes(int format, unsigned width, unsigned x, unsigned n, unsigned* unit, size_t* byte_offset, size_t* bytes)
{
    YuvPackedGeom g;
    int rc;
    if ((rc = yuv_packed_geom(format, g))) return rc;
    if (width == 0 || n == 0) return fail(SRCNN_E_ARG, "zero width %u or count %u", width, n);
    if ((unsigned long long)x + n > width) return fail(SRCNN_E_ARG, "pixels [%u, %u + %u) are not inside a row of %u", x, x, n, width);
    if ((rc = check_yuv_packed_unit(g, width, x, n))) return rc;
    size_t off = 0, len = 0;
    yuv_packed_span(g.rule.kind, width, x, n, off, len);
    if (unit) *unit = yuv_packed_unit(g.rule.kind);
    if (byte_offset) *byte_offset = off;
    if (bytes) *bytes = len;
    return SRCNN_OK;
}

// The chroma columns [cx0, cx1) that cover luma columns [x0, x1) of a packed row (x0 under the unit rule)
struct YuvPackedChromaCols {
    unsigned cx0, cx1;
    YuvPackedChromaCols(int kind, unsigned x0, unsigned x1) : cx0(x0 / yuv_packed_chroma_step(kind)), cx1(yuv_packed_chroma_cols(kind, x1)) {}
};

// The source rectangle of a packed rect in LUMA pixels: the union of the Y path's [ylx, yhx) x [yly, yhy) and the chroma / alpha
// taps' [clx, chx) x [cly, chy) (columns on the chroma grid), widened outward to the unit and cut at w.
inline void yuv_packed_source_union(int kind, unsigned w, unsigned ylx, unsigned yhx, unsigned yly, unsigned yhy, unsigned clx, unsigned chx,
                                    unsigned cly, unsigned chy, unsigned& sx0, unsigned& sy0, unsigned& sw, unsigned& sh)
{
    const unsigned step = yuv_packed_chroma_step(kind), unit = yuv_packed_unit(kind);
    unsigned lx = std::min(ylx, clx * step), hx = std::max(yhx, std::min(chx * step, w));
    lx -= lx % unit;
    hx = std::min(w, (hx + unit - 1) / unit * unit);
    sx0 = lx; sw = hx - lx;
    sy0 = std::min(yly, cly); sh = std::max(yhy, chy) - sy0;
}

// srcnn_yuv_packed_rect_source
inline int yuv_packed_rect_source(int format, unsigned w, unsigned h, float multiply, int filter, unsigned x0, unsigned y0, unsigned rw,
                                  unsigned rh, unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh)
{
    YuvPackedGeom g;
    unsigned dw = 0, dh = 0, ylx, yhx, yly, yhy, clx, chx, cly, chy, ux, uy, uw, uh;
    int rc;
    if ((rc = yuv_packed_geom(format, g))) return rc;
    if (rw == 0 || rh == 0) return fail(SRCNN_E_ARG, "empty rect %ux%u", rw, rh);
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    if ((rc = check_rect_inside(dw, dh, x0, y0, rw, rh))) return rc;
    if ((rc = check_yuv_packed_unit(g, dw, x0, rw))) return rc;
    y_path_rect_source_span(w, h, dw, dh, filter, x0, y0, x0 + rw, y0 + rh, ylx, yhx, yly, yhy);
    const YuvPackedChromaCols cc(g.rule.kind, x0, x0 + rw);
    const int cfilter = chroma_filter(filter);
    axis_source_span(cfilter, g.ccols(dw), g.ccols(w), cc.cx0, cc.cx1, clx, chx);
    axis_source_span(cfilter, dh, h, y0, y0 + rh, cly, chy);
    yuv_packed_source_union(g.rule.kind, w, ylx, yhx, yly, yhy, clx, chx, cly, chy, ux, uy, uw, uh);
    if (sx0) *sx0 = ux;
    if (sy0) *sy0 = uy;
    if (sw) *sw = uw;
    if (sh) *sh = uh;
    return SRCNN_OK;
}

// Whether k_yuvp_window_merge serves chroma output columns [cx0, cx0 + ccols) and rows [y0, y0 + rows): window_tile_fits with the
// tile width that kernel really uses for the kind (60 chroma columns for v210, 20 groups of 3)
inline bool yuvp_window_fits(int kind, const TileAxis& th, const TileAxis& tv, unsigned cx0, unsigned ccols, unsigned y0, unsigned rows)
{
    return axis_tiles_fit(th.first, th.taps, th.max_taps, cx0, ccols, yuv_packed_tile_cols(kind), kPatchW) &&
           axis_tiles_fit(tv.first, tv.taps, tv.max_taps, y0, rows, kTileH, kPatchH);
}

}  // namespace srcnn
