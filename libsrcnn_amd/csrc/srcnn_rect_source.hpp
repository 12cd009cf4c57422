// srcnn_rect_source.hpp -- which part of a source plane a rect of the output depends on, without a device: the geometry behind
// srcnn_y_path_rect_source, srcnn_rgb_rect_source and srcnn_yuv_rect_source.  It needs the contribution-table builder
// (resample_table.hpp) and the argument checks (srcnn_frame_args.hpp) only -- no HIP -- so tests/host/yuv_rect_sanitize.cpp
// runs it under the CPU sanitizers.  Internal.
#pragma once
#include <algorithm>

#include "resample_table.hpp"
#include "srcnn_frame_args.hpp"

namespace srcnn {

// [lo,hi) of the source axis that destination indices [a,b) of the resampled axis read: the taps of the range, read off the
// table; an axis that keeps its size is copied
inline void axis_source_span(int filter, unsigned dst_len, unsigned src_len, unsigned a, unsigned b, unsigned& lo, unsigned& hi)
{
    if (dst_len == src_len) { lo = a; hi = b; return; }
    const AxisTable t = build_axis_table(filter, dst_len, src_len);
    int l = 0x7fffffff, e = 0;
    for (unsigned u = a; u < b; ++u) { l = std::min(l, (int)t.first[u]); e = std::max(e, (int)(t.first[u] + t.taps[u])); }
    lo = (unsigned)l;
    hi = std::min((unsigned)e, src_len);
}

// [lx,hx) x [ly,hy) of the w x h plane that samples [x0,x1) x [y0,y1) of the Y path's dw x dh output depend on: the rect, +-2
// (layer 3) and +-4 (layer 1) cut at the borders, then the resampler's taps.  The rect lies inside the output.
inline void y_path_rect_source_span(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned x0, unsigned y0, unsigned x1,
                                    unsigned y1, unsigned& lx, unsigned& hx, unsigned& ly, unsigned& hy)
{
    const unsigned cax = x0 >= 2 ? x0 - 2 : 0, cbx = std::min(dw, x1 + 2);
    const unsigned uax = cax >= 4 ? cax - 4 : 0, ubx = std::min(dw, cbx + 4);
    const unsigned cay = y0 >= 2 ? y0 - 2 : 0, cby = std::min(dh, y1 + 2);
    const unsigned uay = cay >= 4 ? cay - 4 : 0, uby = std::min(dh, cby + 4);
    axis_source_span(filter, dw, w, uax, ubx, lx, hx);
    axis_source_span(filter, dh, h, uay, uby, ly, hy);
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

}  // namespace srcnn
