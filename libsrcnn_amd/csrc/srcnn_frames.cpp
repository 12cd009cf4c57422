// srcnn_frames.cpp -- the frame calls around the Y path: integer frames in device memory in, integer frames out.
//   include/srcnn_amd_yuv.h          srcnn_yuv420_upscale_dev        8-bit 4:2:0 (I420 / NV12)
//   include/srcnn_amd_yuv_ex.h       srcnn_yuv_upscale_dev           planar / semi-planar, 8-16 bits, 4:2:0 / 4:2:2 / 4:4:4
//   include/srcnn_amd_yuv_packed.h   srcnn_yuv_packed_upscale_dev    YUY2, UYVY, Y210, Y410, v210 ...
//   include/srcnn_amd_rgb.h          srcnn_rgb_upscale_dev           RGB(A), interleaved or planar, 8-16 bits
//   include/srcnn_amd_rgb_rect.h     srcnn_rgb_upscale_rect_dev      one rectangle of that call's output, at the rect's cost
//   include/srcnn_amd_yuv_rect.h     srcnn_yuv_upscale_rect_dev      one rectangle of srcnn_yuv_upscale_dev's output, likewise
//   include/srcnn_amd_yuv_packed_rect.h  srcnn_yuv_packed_upscale_rect_dev  one rectangle of srcnn_yuv_packed_upscale_dev's, likewise
//
// Every call has the same skeleton: refuse what the arguments rule out before any device lookup (srcnn_frame_args.hpp), lay
// the float planes out in ws.planes (PlaneArena), unpack the source (srcnn_yuv_planes.hip, srcnn_yuv_packed.hip,
// srcnn_rgb.hip), resample chroma and alpha with chroma_filter(), and produce Y' band by band (for_each_y_band): the Y path
// of srcnn_capi.cpp into a float band, then the call's own pack of that band.  The state shared with the other translation
// units is srcnn_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/srcnn_amd_rect.h"
#include "../../include/srcnn_amd_rgb_rect.h"
#include "../../include/srcnn_amd_yuv_packed_rect.h"
#include "../../include/srcnn_amd_yuv_rect.h"
#include "srcnn_frame_args.hpp"
#include "srcnn_host.hpp"
#include "srcnn_rect_source.hpp"
#include "srcnn_rgb.h"
#include "srcnn_window_tile.h"
#include "srcnn_yuv.h"

namespace srcnn {

namespace {

// Float planes in ws.planes, in the order they are taken; each start is rounded up to 64 floats (16-byte accesses in the
// conversion kernels).
struct PlaneArena {
    size_t n = 0;           // floats needed so far
    size_t take(size_t k) { const size_t o = (n + 63) & ~(size_t)63; n = o + k; return o; }
};

// Y' in bands of `band` rows: the Y path writes rows [a, b) to yband, then after(a, b) packs them into the destination.
template <class After>
int for_each_y_band(Call& c, const YSource& ysrc, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned band,
                    float* yband, After after)
{
    for (unsigned a = 0; a < dh; a += band) {
        const unsigned b = std::min(dh, a + band);
        int rc;
        if ((rc = y_path_rows(c, ysrc, w, h, dw, dh, filter, a, b, yband))) return rc;
        if ((rc = after(a, b))) return rc;
    }
    HIP_TRY(hipGetLastError());
    return SRCNN_OK;
}

// unpack -> chroma resample + pack (whole planes) -> Y' band by band.
int yuv_frame(Call& c, const YuvGeom& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const YuvPlane in[3],
              const YuvPlane out[3])
{
    Workspace& ws = *c.ws;
    const unsigned cw = g.ccols(w), ch = g.crows(h), dcw = g.ccols(dw), dch = g.crows(dh);
    const unsigned band = y_path_pass_rows(c, dw, dh);
    PlaneArena A;
    const size_t o_y = A.take((size_t)w * h), o_u = A.take((size_t)cw * ch), o_v = A.take((size_t)cw * ch);
    const size_t o_cu = A.take((size_t)dcw * dch), o_cv = A.take((size_t)dcw * dch), o_band = A.take((size_t)dw * band);
    int rc;
    if ((rc = ws.grow(ws.planes, A.n))) return rc;
    float* P = ws.planes.data();
    const Yuv16Rule* rule = g.bps == 2 ? &g.rule : nullptr;
    auto unpack = [&](const YuvPlane& p, unsigned pw, unsigned ph, bool luma, float* d0, float* d1) {
        launch_plane_unpack(p.lo, p.pitch, pw, ph, d1 != nullptr, rule, luma, d0, d1, c.s);
    };
    auto pack = [&](const float* s0, const float* s1, unsigned pw, unsigned ph, bool sat, const YuvPlane& p, unsigned row0) {
        launch_plane_pack(s0, s1, pw, ph, sat, rule, const_cast<unsigned char*>(p.lo), p.pitch, row0, c.s);
    };
    unpack(in[0], w, h, true, P + o_y, nullptr);
    if (g.semi) unpack(in[1], cw, ch, false, P + o_u, P + o_v);
    else {
        unpack(in[1], cw, ch, false, P + o_u, nullptr);
        unpack(in[2], cw, ch, false, P + o_v, nullptr);
    }
    const int cfilter = chroma_filter(filter);
    if ((rc = resample_rows_range(c, P + o_u, cw, ch, dcw, dch, cfilter, 0, dch, P + o_cu))) return rc;
    if ((rc = resample_rows_range(c, P + o_v, cw, ch, dcw, dch, cfilter, 0, dch, P + o_cv))) return rc;
    if (g.semi) pack(P + o_cu, P + o_cv, dcw, dch, true, out[1], 0);
    else {
        pack(P + o_cu, nullptr, dcw, dch, true, out[1], 0);
        pack(P + o_cv, nullptr, dcw, dch, true, out[2], 0);
    }
    return for_each_y_band(c, YSource::from_plane(P + o_y), w, h, dw, dh, filter, band, P + o_band, [&](unsigned a, unsigned b) {
        pack(P + o_band, nullptr, dw, b - a, false, out[0], a);
        return SRCNN_OK;
    });
}

// unpack -> chroma / alpha resample (whole planes) -> Y' band by band, each band packed with the same rows of the finished
// chroma and alpha planes (a packed row mixes them, and every packed format has one chroma row per luma row).
int yuv_packed_frame(Call& c, const YuvPackedGeom& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                     const YuvPlane& in, const YuvPlane& out)
{
    Workspace& ws = *c.ws;
    const unsigned cw = g.ccols(w), dcw = g.ccols(dw);
    const unsigned band = y_path_pass_rows(c, dw, dh);
    // [Y U V (A) at source size] [U' V' (A') at output size] [Y' of one band]
    PlaneArena A;
    const size_t o_y = A.take((size_t)w * h), o_u = A.take((size_t)cw * h), o_v = A.take((size_t)cw * h);
    const size_t o_a = A.take(g.alpha ? (size_t)w * h : 0);
    const size_t o_cu = A.take((size_t)dcw * dh), o_cv = A.take((size_t)dcw * dh), o_ca = A.take(g.alpha ? (size_t)dw * dh : 0);
    const size_t o_band = A.take((size_t)dw * band);
    int rc;
    if ((rc = ws.grow(ws.planes, A.n))) return rc;
    float* P = ws.planes.data();
    launch_yuvp_unpack(in.lo, in.pitch, w, h, g.rule, P + o_y, P + o_u, P + o_v, g.alpha ? P + o_a : nullptr, c.s);
    const int cfilter = chroma_filter(filter);
    if ((rc = resample_rows_range(c, P + o_u, cw, h, dcw, dh, cfilter, 0, dh, P + o_cu))) return rc;
    if ((rc = resample_rows_range(c, P + o_v, cw, h, dcw, dh, cfilter, 0, dh, P + o_cv))) return rc;
    if (g.alpha && (rc = resample_rows_range(c, P + o_a, w, h, dw, dh, cfilter, 0, dh, P + o_ca))) return rc;
    unsigned char* d = const_cast<unsigned char*>(out.lo);
    return for_each_y_band(c, YSource::from_plane(P + o_y), w, h, dw, dh, filter, band, P + o_band, [&](unsigned a, unsigned b) {
        launch_yuvp_pack(P + o_band, P + o_cu + (size_t)a * dcw, P + o_cv + (size_t)a * dcw, g.alpha ? P + o_ca + (size_t)a * dw : nullptr,
                         dw, b - a, g.rule, d, out.pitch, a, c.s);
        return SRCNN_OK;
    });
}

// The planes of an RGB(A) call as the conversion launchers take them (interleaved: plane 0 only)
struct RgbPlanes {
    const unsigned char* src[4] = {nullptr, nullptr, nullptr, nullptr};
    unsigned char* dst[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t spitch[4] = {0, 0, 0, 0}, dpitch[4] = {0, 0, 0, 0};
    RgbPlanes(const RgbRule& g, const YuvPlane in[4], const YuvPlane out[4])
    {
        for (int k = 0; k < (g.planar ? g.ch : 1); ++k) {
            src[k] = in[k].lo; spitch[k] = in[k].pitch;
            dst[k] = const_cast<unsigned char*>(out[k].lo); dpitch[k] = out[k].pitch;
        }
    }
};

// The reference's own format (8-bit interleaved R,G,B[,A], tight rows, an up-scale in both axes) goes through the fused shell
// of srcnn_process_u8: Y' from the interleaved source (k_rs2d), then the merge with on-the-fly chroma -- no float plane of
// source or destination size.  Everything else: unpack -> per band { Y path, chroma / alpha resample, pack }.  conv.lo == NULL:
// no truncated Y' plane.
int rgb_frame(Call& c, const RgbRule& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const YuvPlane in[4],
              const YuvPlane out[4], const YuvPlane& conv)
{
    Workspace& ws = *c.ws;
    const int cfilter = chroma_filter(filter);
    const unsigned band = y_path_pass_rows(c, dw, dh);
    int rc;
    const bool tight = in[0].pitch == in[0].row_bytes && out[0].pitch == out[0].row_bytes && (!conv.lo || conv.pitch == conv.row_bytes);
    // (as in process_share: the switches that force the plane resamplers select the plane shell as well)
    bool fused_shell = g.bps == 1 && !g.planar && !g.bgr && tight && !settings().shell_unfused && !settings().resample_2pass && dw > w && dh > h;
    TableRef cv, ch_, yv, yh;
    if (fused_shell) {
        if ((rc = get_table(c, cfilter, dh, h, cv))) return rc;
        if ((rc = get_table(c, cfilter, dw, w, ch_))) return rc;
        if ((rc = get_table(c, filter, dh, h, yv))) return rc;
        if ((rc = get_table(c, filter, dw, w, yh))) return rc;
        fused_shell = rs2d_fits(1, (int)w, (int)h, (int)dw, (int)dh, 0, (int)dh, yv->view(), yh->view()) &&
                      rs2d_fits(g.ch - 1, (int)w, (int)h, (int)dw, (int)dh, 0, (int)dh, cv->view(), ch_->view());
    }
    if (fused_shell) {
        if ((rc = ws.grow(ws.planes, (size_t)dw * band))) return rc;
        float* yp = ws.planes.data();
        unsigned char* d_out = const_cast<unsigned char*>(out[0].lo);
        unsigned char* d_conv = const_cast<unsigned char*>(conv.lo);
        return for_each_y_band(c, YSource::from_rgb(in[0].lo, g.ch), w, h, dw, dh, filter, band, yp, [&](unsigned a, unsigned b) {
            const size_t p0 = (size_t)a * dw;
            if (!launch_merge_fused(in[0].lo, (int)w, (int)h, g.ch, yp, d_out + p0 * g.ch, d_conv ? d_conv + p0 : nullptr, (int)dw,
                                    (int)dh, (int)a, (int)(b - a), cv->view(), ch_->view(), c.s))
                return fail(SRCNN_E_UNSUPPORTED, "fused colour shell refused a shape it was selected for");
            return SRCNN_OK;
        });
    }
    // [Y Cb Cr (A) at source size] [Y' Cb' Cr' (A') of one band]
    PlaneArena A;
    float* sp[4] = {nullptr, nullptr, nullptr, nullptr};
    float* dp[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t so[4], bo[4];
    for (int k = 0; k < g.ch; ++k) so[k] = A.take((size_t)w * h);
    for (int k = 0; k < g.ch; ++k) bo[k] = A.take((size_t)dw * band);
    if ((rc = ws.grow(ws.planes, A.n))) return rc;
    for (int k = 0; k < g.ch; ++k) { sp[k] = ws.planes.data() + so[k]; dp[k] = ws.planes.data() + bo[k]; }
    const RgbPlanes pl(g, in, out);
    launch_rgb_unpack(g, pl.src, pl.spitch, w, h, sp, c.s);
    return for_each_y_band(c, YSource::from_plane(sp[0]), w, h, dw, dh, filter, band, dp[0], [&](unsigned a, unsigned b) {
        for (int k = 1; k < g.ch; ++k)
            if (int rk = resample_rows_range(c, sp[k], w, h, dw, dh, cfilter, a, b, dp[k])) return rk;
        launch_rgb_pack(g, dp, dw, b - a, pl.dst, pl.dpitch, a, const_cast<unsigned char*>(conv.lo), conv.pitch, c.s);
        return SRCNN_OK;
    });
}

// [lo, hi) of a source axis that destination indices [a, b) read with `filter`, off the call's cached table (an axis that keeps
// its size is copied): what srcnn_rgb_rect_source reports, without building a table per call
int axis_span(Call& c, int filter, unsigned dst_len, unsigned src_len, unsigned a, unsigned b, unsigned& lo, unsigned& hi)
{
    if (dst_len == src_len) { lo = a; hi = b; return SRCNN_OK; }
    TableRef t;
    int rc;
    if ((rc = get_table(c, filter, dst_len, src_len, t))) return rc;
    t->source_span(a, b, lo, hi);
    return SRCNN_OK;
}

// The source rectangles of a rect, each [lx, hx) x [ly, hy): what the Y path reads of the luma plane (the halo of the luma rect,
// then the taps of `filter`), and what the taps of `cfilter` read of a chroma / alpha plane for the chroma rect
struct RectSource {
    unsigned ylx, yhx, yly, yhy;
    unsigned clx, chx, cly, chy;
    unsigned yw() const { return yhx - ylx; }
    unsigned yh() const { return yhy - yly; }
};

// luma: w x h -> dw x dh, rect [x0, x1) x [y0, y1); chroma: cw x ch -> dcw x dch, rect [cx0, cx1) x [cy0, cy1)
int rect_source(Call& c, int filter, int cfilter, unsigned w, unsigned h, unsigned dw, unsigned dh, unsigned cw, unsigned ch, unsigned dcw,
                unsigned dch, unsigned x0, unsigned y0, unsigned x1, unsigned y1, unsigned cx0, unsigned cy0, unsigned cx1, unsigned cy1,
                RectSource& r)
{
    int rc;
    const HaloSpan vx = y_path_halo(dw, x0, x1), vy = y_path_halo(dh, y0, y1);
    if ((rc = axis_span(c, filter, dw, w, vx.ua, vx.ub, r.ylx, r.yhx))) return rc;
    if ((rc = axis_span(c, filter, dh, h, vy.ua, vy.ub, r.yly, r.yhy))) return rc;
    if ((rc = axis_span(c, cfilter, dcw, cw, cx0, cx1, r.clx, r.chx))) return rc;
    if ((rc = axis_span(c, cfilter, dch, ch, cy0, cy1, r.cly, r.chy))) return rc;
    return SRCNN_OK;
}

// Y' of the rect [x0, x1) x [y0, y1) in bands of `band` rows: the window Y path writes rows [a, b) to yband (tight, x1 - x0
// floats per row) from ysrc, the sw x sh float window of the Y plane whose first sample is (sx, sy); then after(a, b)
template <class After>
int for_each_rect_band(Call& c, const float* ysrc, unsigned sx, unsigned sy, unsigned sw, unsigned sh, unsigned w, unsigned h, unsigned dw,
                       unsigned dh, int filter, unsigned x0, unsigned y0, unsigned x1, unsigned y1, unsigned band, float* yband, After after)
{
    const bool whole = sx == 0 && sy == 0 && sw == w && sh == h;
    for (unsigned a = y0; a < y1; a += band) {
        const unsigned b = std::min(y1, a + band);
        int rc;
        if ((rc = y_path_rect(c, ysrc, sw, sx, sy, w, h, dw, dh, filter, x0, a, x1, b, yband, x1 - x0, whole))) return rc;
        if ((rc = after(a, b))) return rc;
    }
    HIP_TRY(hipGetLastError());
    return SRCNN_OK;
}

// The rect [x0, x1) x [y0, y1) of what rgb_frame writes, at the cost of the rect: every step works on a window.  out[] and conv
// are the rect's own planes (pixel (x0, y0) first).  Y' comes from the window Y path (y_path_rect) band by band, in its bands.
//   up-scale in both axes, tables of at most 8 taps:  k_rgb_window_y over the Y path's source rectangle -> per band
//       { y_path_rect, k_rgb_window_merge: chroma / alpha resampled from the integer source, merge, store }
//   everything else, and SRCNN_RGB_RECT_UNFUSED=1:     the plane route over the window: unpack of the source rectangle (the
//       union of the Y path's and the chroma taps') -> per band { y_path_rect, resample_window per chroma / alpha plane, pack }
// Both read no sample outside the rectangle srcnn_rgb_rect_source reports, and both give the bytes of rgb_frame.
// (Declared in srcnn_host.hpp: the single items of the RGB(A) rect list call, srcnn_rgb_rect_list_call.cpp, run it too.)
}  // namespace

int rgb_rect(Call& c, const RgbRule& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const YuvPlane in[4],
             const YuvPlane out[4], const YuvPlane& conv, unsigned x0, unsigned y0, unsigned x1, unsigned y1)
{
    Workspace& ws = *c.ws;
    const int cfilter = chroma_filter(filter);
    const unsigned rw = x1 - x0;
    const unsigned band = y_path_pass_rows(c, y_path_halo(dw, x0, x1).width(), y1 - y0);
    int rc;
    RectSource r;
    if ((rc = rect_source(c, filter, cfilter, w, h, dw, dh, w, h, dw, dh, x0, y0, x1, y1, x0, y0, x1, y1, r))) return rc;
    const RgbPlanes pl(g, in, out);
    unsigned char* d_conv = const_cast<unsigned char*>(conv.lo);
    TraceRange tr("srcnn rgb rect [%u,%u)x[%u,%u) of %ux%u", x0, x1, y0, y1, dw, dh);

    TableRef cv, ch_;
    bool fused = !settings().rgb_rect_unfused && dw > w && dh > h;
    if (fused) {
        if ((rc = get_table(c, cfilter, dh, h, cv))) return rc;
        if ((rc = get_table(c, cfilter, dw, w, ch_))) return rc;
        for (unsigned a = y0; a < y1 && fused; a += band)
            fused = window_tile_fits(ch_->view(), cv->view(), x0, rw, a, std::min(y1, a + band) - a);
    }
    PlaneArena A;
    if (fused) {
        // [Y of the Y path's source rectangle] [Y' of one band]
        const size_t o_y = A.take((size_t)r.yw() * r.yh()), o_band = A.take((size_t)rw * band);
        if ((rc = ws.grow(ws.planes, A.n))) return rc;
        float* P = ws.planes.data();
        launch_rgb_window_y(g, pl.src, pl.spitch, r.ylx, r.yly, r.yw(), r.yh(), P + o_y, c.s);
        return for_each_rect_band(c, P + o_y, r.ylx, r.yly, r.yw(), r.yh(), w, h, dw, dh, filter, x0, y0, x1, y1, band, P + o_band,
                                  [&](unsigned a, unsigned b) {
            launch_rgb_window_merge(g, pl.src, pl.spitch, w, h, P + o_band, x0, a, rw, b - a, ch_->view(), cv->view(), pl.dst, pl.dpitch,
                                    a - y0, d_conv, conv.pitch, c.s);
            return SRCNN_OK;
        });
    }
    // [Y Cb Cr (A) of the source rectangle] [Y' Cb' Cr' (A') of one band]
    const unsigned ux = std::min(r.ylx, r.clx), uy = std::min(r.yly, r.cly);
    const unsigned uw = std::max(r.yhx, r.chx) - ux, uh = std::max(r.yhy, r.chy) - uy;
    float* sp[4] = {nullptr, nullptr, nullptr, nullptr};
    float* dp[4] = {nullptr, nullptr, nullptr, nullptr};
    size_t so[4], bo[4];
    for (int k = 0; k < g.ch; ++k) so[k] = A.take((size_t)uw * uh);
    for (int k = 0; k < g.ch; ++k) bo[k] = A.take((size_t)rw * band);
    if ((rc = ws.grow(ws.planes, A.n))) return rc;
    for (int k = 0; k < g.ch; ++k) { sp[k] = ws.planes.data() + so[k]; dp[k] = ws.planes.data() + bo[k]; }
    const unsigned char* wsrc[4] = {nullptr, nullptr, nullptr, nullptr};      // the planes at the source rectangle's first sample
    for (int k = 0; k < (g.planar ? g.ch : 1); ++k)
        wsrc[k] = pl.src[k] + (size_t)uy * pl.spitch[k] + (size_t)ux * g.bps * (g.planar ? 1 : g.ch);
    launch_rgb_unpack(g, wsrc, pl.spitch, uw, uh, sp, c.s);
    return for_each_rect_band(c, sp[0], ux, uy, uw, uh, w, h, dw, dh, filter, x0, y0, x1, y1, band, dp[0], [&](unsigned a, unsigned b) {
        for (int k = 1; k < g.ch; ++k)
            if (int rk = resample_window(c, sp[k], uw, ux, uy, w, h, dw, dh, cfilter, x0, x1, a, b, dp[k])) return rk;
        launch_rgb_pack(g, dp, rw, b - a, pl.dst, pl.dpitch, a - y0, d_conv, conv.pitch, c.s);
        return SRCNN_OK;
    });
}

namespace {

// The luma rect [x0, x1) x [y0, y1) and the chroma samples that cover it (cr) of what yuv_frame writes, at the cost of the rect.
// out[] are the rect's own planes (luma sample (x0, y0) and chroma sample (cr.cx0, cr.cy0) first).
//   Y':      unpack of the Y path's source rectangle -> per band { y_path_rect, pack }
//   chroma:  once for the rect, not per band.  Up-scale in both axes of the CHROMA grid, tables of at most 8 taps:
//            k_yuv_window_chroma from the integer source.  Everything else, and SRCNN_YUV_RECT_UNFUSED=1: the plane route over the
//            window: unpack of the chroma source rectangle -> resample_window per plane -> pack.
// Both read no sample outside the rectangles srcnn_yuv_rect_source reports, and both give the bytes of yuv_frame.
// (Declared in srcnn_host.hpp: the single items of the YUV rect list call, srcnn_yuv_rect_list_call.cpp, run it too.)
}  // namespace

int yuv_rect(Call& c, const YuvGeom& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const YuvPlane in[3],
             const YuvPlane out[3], unsigned x0, unsigned y0, unsigned x1, unsigned y1)
{
    Workspace& ws = *c.ws;
    const int cfilter = chroma_filter(filter);
    const YuvChromaRect cr(g, x0, y0, x1, y1);
    const unsigned rw = x1 - x0, crw = cr.cx1 - cr.cx0, crh = cr.cy1 - cr.cy0;
    const unsigned cw = g.ccols(w), ch = g.crows(h), dcw = g.ccols(dw), dch = g.crows(dh);
    const unsigned band = y_path_pass_rows(c, y_path_halo(dw, x0, x1).width(), y1 - y0);
    const unsigned spp = g.semi ? 2 : 1;                 // samples per column of a chroma plane
    const int ncp = g.semi ? 1 : 2;                      // chroma planes in memory
    int rc;
    RectSource r;
    if ((rc = rect_source(c, filter, cfilter, w, h, dw, dh, cw, ch, dcw, dch, x0, y0, x1, y1, cr.cx0, cr.cy0, cr.cx1, cr.cy1, r))) return rc;
    const unsigned cuw = r.chx - r.clx, cuh = r.chy - r.cly;
    TraceRange tr("srcnn yuv rect [%u,%u)x[%u,%u) of %ux%u", x0, x1, y0, y1, dw, dh);

    TableRef cv, ch_;
    bool fused = !settings().yuv_rect_unfused && dcw > cw && dch > ch;
    if (fused) {
        if ((rc = get_table(c, cfilter, dch, ch, cv))) return rc;
        if ((rc = get_table(c, cfilter, dcw, cw, ch_))) return rc;
        fused = window_tile_fits(ch_->view(), cv->view(), cr.cx0, crw, cr.cy0, crh);
    }
    // [Y of the Y path's source rectangle] [Y' of one band] and, on the plane route, [U V of the chroma source rectangle] [U' V']
    PlaneArena A;
    const size_t o_y = A.take((size_t)r.yw() * r.yh()), o_band = A.take((size_t)rw * band);
    size_t o_c[2] = {0, 0}, o_dc[2] = {0, 0};
    if (!fused) {
        for (int k = 0; k < 2; ++k) o_c[k] = A.take((size_t)cuw * cuh);
        for (int k = 0; k < 2; ++k) o_dc[k] = A.take((size_t)crw * crh);
    }
    if ((rc = ws.grow(ws.planes, A.n))) return rc;
    float* P = ws.planes.data();
    const Yuv16Rule* rule = g.bps == 2 ? &g.rule : nullptr;
    unsigned char* dst[3];
    for (int k = 0; k < 3; ++k) dst[k] = const_cast<unsigned char*>(out[k].lo);

    if (fused) {
        const unsigned char* csrc[2] = {in[1].lo, in[2].lo};
        const size_t cspitch[2] = {in[1].pitch, in[2].pitch}, cdpitch[2] = {out[1].pitch, out[2].pitch};
        launch_yuv_window_chroma(csrc, cspitch, cw, ch, g.semi, rule, cr.cx0, cr.cy0, crw, crh, ch_->view(), cv->view(), dst + 1, cdpitch, c.s);
    } else {
        for (int k = 0; k < ncp; ++k)                    // the planes at the chroma source rectangle's first sample
            launch_plane_unpack(in[1 + k].lo + (size_t)r.cly * in[1 + k].pitch + (size_t)r.clx * g.bps * spp, in[1 + k].pitch, cuw, cuh, g.semi,
                                rule, false, P + o_c[k], g.semi ? P + o_c[1] : nullptr, c.s);
        for (int k = 0; k < 2; ++k)
            if ((rc = resample_window(c, P + o_c[k], cuw, r.clx, r.cly, cw, ch, dcw, dch, cfilter, cr.cx0, cr.cx1, cr.cy0, cr.cy1, P + o_dc[k]))) return rc;
        for (int k = 0; k < ncp; ++k)
            launch_plane_pack(P + o_dc[k], g.semi ? P + o_dc[1] : nullptr, crw, crh, true, rule, dst[1 + k], out[1 + k].pitch, 0, c.s);
    }

    launch_plane_unpack(in[0].lo + (size_t)r.yly * in[0].pitch + (size_t)r.ylx * g.bps, in[0].pitch, r.yw(), r.yh(), false, rule, true, P + o_y,
                        nullptr, c.s);
    return for_each_rect_band(c, P + o_y, r.ylx, r.yly, r.yw(), r.yh(), w, h, dw, dh, filter, x0, y0, x1, y1, band, P + o_band,
                              [&](unsigned a, unsigned b) {
        launch_plane_pack(P + o_band, nullptr, rw, b - a, false, rule, dst[0], out[0].pitch, a - y0, c.s);
        return SRCNN_OK;
    });
}

// Luma columns [x0, x1) (under the unit rule) of rows [y0, y1) of what yuv_packed_frame writes, at the cost of the rect.  out is
// the rect's own row segments: out.row_bytes bytes (yuv_packed_span of the rect) per row, the byte of pixel (x0, y0) first.  A
// packed row mixes luma and chroma, so chroma and alpha are merged per band of Y', not once per rect.
//   up-scale in both axes of the CHROMA grid, tables of at most 8 taps:  k_yuvp_window_y over the Y path's source rectangle ->
//       per band { y_path_rect, k_yuvp_window_merge: chroma / alpha resampled from the packed source, merged, encoded, stored }
//   everything else, and SRCNN_YUV_PACKED_RECT_UNFUSED=1:  the plane route over the window: unpack of the unit-aligned source
//       rectangle -> per band { y_path_rect, resample_window per chroma / alpha plane, pack into the row segments }
// Both read no byte outside the rectangle srcnn_yuv_packed_rect_source reports, and both give the bytes of yuv_packed_frame.
// (Declared in srcnn_host.hpp: the single items of the packed rect list call, srcnn_yuv_packed_rect_list_call.cpp, run it too.)
int yuv_packed_rect(Call& c, const YuvPackedGeom& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const YuvPlane& in,
                    const YuvPlane& out, unsigned x0, unsigned y0, unsigned x1, unsigned y1)
{
    Workspace& ws = *c.ws;
    const int kind = g.rule.kind;
    const int cfilter = chroma_filter(filter);
    const YuvPackedChromaCols cc(kind, x0, x1);
    const unsigned rw = x1 - x0, crw = cc.cx1 - cc.cx0;
    const unsigned cw = g.ccols(w), dcw = g.ccols(dw);
    const unsigned band = y_path_pass_rows(c, y_path_halo(dw, x0, x1).width(), y1 - y0);
    int rc;
    RectSource r;
    if ((rc = rect_source(c, filter, cfilter, w, h, dw, dh, cw, h, dcw, dh, x0, y0, x1, y1, cc.cx0, y0, cc.cx1, y1, r))) return rc;
    unsigned char* dst = const_cast<unsigned char*>(out.lo);
    TraceRange tr("srcnn yuv packed rect [%u,%u)x[%u,%u) of %ux%u", x0, x1, y0, y1, dw, dh);

    TableRef cv, ch_;
    bool fused = !settings().yuv_packed_rect_unfused && dcw > cw && dh > h;
    if (fused) {
        if ((rc = get_table(c, cfilter, dh, h, cv))) return rc;
        if ((rc = get_table(c, cfilter, dcw, cw, ch_))) return rc;
        const DevAxisTable th = ch_->view(), tv = cv->view();
        for (unsigned a = y0; a < y1 && fused; a += band)
            fused = yuvp_window_fits(kind, TileAxis{th.h_first, th.h_taps, th.max_taps}, TileAxis{tv.h_first, tv.h_taps, tv.max_taps}, cc.cx0, crw,
                                     a, std::min(y1, a + band) - a);
    }
    PlaneArena A;
    if (fused) {
        // [Y of the Y path's source rectangle] [Y' of one band]
        const size_t o_y = A.take((size_t)r.yw() * r.yh()), o_band = A.take((size_t)rw * band);
        if ((rc = ws.grow(ws.planes, A.n))) return rc;
        float* P = ws.planes.data();
        launch_yuvp_window_y(g.rule, in.lo, in.pitch, w, r.ylx, r.yly, r.yw(), r.yh(), P + o_y, c.s);
        return for_each_rect_band(c, P + o_y, r.ylx, r.yly, r.yw(), r.yh(), w, h, dw, dh, filter, x0, y0, x1, y1, band, P + o_band,
                                  [&](unsigned a, unsigned b) {
            launch_yuvp_window_merge(g.rule, in.lo, in.pitch, w, h, P + o_band, cc.cx0, a, rw, crw, b - a, ch_->view(), cv->view(), dst, out.pitch,
                                     a - y0, out.row_bytes, c.s);
            return SRCNN_OK;
        });
    }
    // [Y U V (A) of the unit-aligned source rectangle] [Y' U' V' (A') of one band]
    unsigned ux, uy, uw, uh;
    yuv_packed_source_union(kind, w, r.ylx, r.yhx, r.yly, r.yhy, r.clx, r.chx, r.cly, r.chy, ux, uy, uw, uh);
    const unsigned cuw = g.ccols(uw), cux = ux / yuv_packed_chroma_step(kind);     // the chroma columns of that rectangle
    const size_t o_y = A.take((size_t)uw * uh), o_u = A.take((size_t)cuw * uh), o_v = A.take((size_t)cuw * uh);
    const size_t o_a = A.take(g.alpha ? (size_t)uw * uh : 0);
    const size_t o_band = A.take((size_t)rw * band), o_cu = A.take((size_t)crw * band), o_cv = A.take((size_t)crw * band);
    const size_t o_ca = A.take(g.alpha ? (size_t)rw * band : 0);
    if ((rc = ws.grow(ws.planes, A.n))) return rc;
    float* P = ws.planes.data();
    size_t soff = 0, sbytes = 0;
    yuv_packed_span(kind, w, ux, uw, soff, sbytes);
    launch_yuvp_unpack(in.lo + (size_t)uy * in.pitch + soff, in.pitch, uw, uh, g.rule, P + o_y, P + o_u, P + o_v, g.alpha ? P + o_a : nullptr, c.s);
    return for_each_rect_band(c, P + o_y, ux, uy, uw, uh, w, h, dw, dh, filter, x0, y0, x1, y1, band, P + o_band, [&](unsigned a, unsigned b) {
        int rk;
        if ((rk = resample_window(c, P + o_u, cuw, cux, uy, cw, h, dcw, dh, cfilter, cc.cx0, cc.cx1, a, b, P + o_cu))) return rk;
        if ((rk = resample_window(c, P + o_v, cuw, cux, uy, cw, h, dcw, dh, cfilter, cc.cx0, cc.cx1, a, b, P + o_cv))) return rk;
        if (g.alpha && (rk = resample_window(c, P + o_a, uw, ux, uy, w, h, dw, dh, cfilter, x0, x1, a, b, P + o_ca))) return rk;
        launch_yuvp_pack(P + o_band, P + o_cu, P + o_cv, g.alpha ? P + o_ca : nullptr, rw, b - a, g.rule, dst, out.pitch, a - y0, c.s, out.row_bytes);
        return SRCNN_OK;
    });
}

}  // namespace srcnn

using namespace srcnn;

extern "C" {

// ---- 8-bit YUV 4:2:0 frames (include/srcnn_amd_yuv.h) ----
int srcnn_yuv_abi_version(void) { return SRCNN_AMD_YUV_VERSION; }

int srcnn_yuv420_upscale_dev(int format, unsigned w, unsigned h, float multiply, int filter,
                             const unsigned char* const src[3], const size_t src_pitch[3],
                             unsigned char* const dst[3], const size_t dst_pitch[3], void* stream)
{
    if (format != SRCNN_YUV_I420 && format != SRCNN_YUV_NV12) return fail(SRCNN_E_ARG, "unknown YUV format %d", format);
    YuvGeom g;                              // 8-bit 4:2:0
    g.semi = format == SRCNN_YUV_NV12;
    unsigned dw = 0, dh = 0;
    YuvPlane in[3], out[3];
    int rc;
    if ((rc = check_yuv_args(g, w, h, multiply, filter, reinterpret_cast<const void* const*>(src), src_pitch,
                             reinterpret_cast<void* const*>(dst), dst_pitch, dw, dh, in, out))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    TraceRange tr("srcnn yuv420 %ux%u -> %ux%u", w, h, dw, dh);
    return yuv_frame(sc.c, g, w, h, dw, dh, filter, in, out);
}

// ---- YUV frames of any supported depth / chroma format (include/srcnn_amd_yuv_ex.h) ----
int srcnn_yuv_ex_abi_version(void) { return SRCNN_AMD_YUV_EX_VERSION; }

int srcnn_yuv_plane_size(const srcnn_yuv_format* fmt, unsigned w, unsigned h, int plane, unsigned* cols, unsigned* rows,
                         size_t* row_bytes)
{
    YuvGeom g;
    int rc;
    if ((rc = yuv_geom_from_format(fmt, g))) return rc;
    if (w == 0 || h == 0) return fail(SRCNN_E_ARG, "zero dimension %ux%u", w, h);
    if (plane < 0 || plane > 2) return fail(SRCNN_E_ARG, "plane %d", plane);
    unsigned pc = w, pr = h;
    size_t rb = (size_t)g.bps * w;
    if (plane > 0) {
        pc = g.ccols(w), pr = g.crows(h);
        rb = (size_t)g.bps * pc * (g.semi ? 2 : 1);
        if (g.semi && plane == 2) pc = pr = 0, rb = 0;
    }
    if (cols) *cols = pc;
    if (rows) *rows = pr;
    if (row_bytes) *row_bytes = rb;
    return SRCNN_OK;
}

int srcnn_yuv_upscale_dev(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                          const void* const src[3], const size_t src_pitch[3],
                          void* const dst[3], const size_t dst_pitch[3], void* stream)
{
    YuvGeom g;
    unsigned dw = 0, dh = 0;
    YuvPlane in[3], out[3];
    int rc;
    if ((rc = yuv_geom_from_format(fmt, g))) return rc;
    if ((rc = check_yuv_args(g, w, h, multiply, filter, src, src_pitch, dst, dst_pitch, dw, dh, in, out))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    TraceRange tr("srcnn yuv %ux%u -> %ux%u", w, h, dw, dh);
    return yuv_frame(sc.c, g, w, h, dw, dh, filter, in, out);
}

// ---- packed YUV frames (include/srcnn_amd_yuv_packed.h) ----
int srcnn_yuv_packed_abi_version(void) { return SRCNN_AMD_YUV_PACKED_VERSION; }

int srcnn_yuv_packed_row_bytes(int format, unsigned w, size_t* row_bytes, unsigned* alignment)
{
    YuvPackedGeom g;
    int rc;
    if ((rc = yuv_packed_geom(format, g))) return rc;
    if (w == 0) return fail(SRCNN_E_ARG, "zero width");
    if (row_bytes) *row_bytes = g.row_bytes(w);
    if (alignment) *alignment = g.align;
    return SRCNN_OK;
}

int srcnn_yuv_packed_upscale_dev(int format, unsigned w, unsigned h, float multiply, int filter, const void* src, size_t src_pitch,
                                 void* dst, size_t dst_pitch, void* stream)
{
    YuvPackedGeom g;
    unsigned dw = 0, dh = 0;
    YuvPlane in, out;
    int rc;
    if ((rc = yuv_packed_geom(format, g))) return rc;
    if ((rc = check_yuv_packed_args(g, w, h, multiply, filter, src, src_pitch, dst, dst_pitch, dw, dh, in, out))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    TraceRange tr("srcnn yuv packed %ux%u -> %ux%u", w, h, dw, dh);
    return yuv_packed_frame(sc.c, g, w, h, dw, dh, filter, in, out);
}

// ---- RGB(A) images in device memory (include/srcnn_amd_rgb.h) ----
int srcnn_rgb_abi_version(void) { return SRCNN_AMD_RGB_VERSION; }

int srcnn_rgb_plane_size(const srcnn_rgb_format* fmt, unsigned w, unsigned h, int plane, unsigned* cols, unsigned* rows,
                         size_t* row_bytes)
{
    RgbRule g;
    int rc;
    if ((rc = rgb_rule_from_format(fmt, g))) return rc;
    if (w == 0 || h == 0) return fail(SRCNN_E_ARG, "zero dimension %ux%u", w, h);
    if (plane < 0 || plane > 3) return fail(SRCNN_E_ARG, "plane %d", plane);
    const bool used = g.planar ? plane < g.ch : plane == 0;
    if (cols) *cols = used ? w : 0;
    if (rows) *rows = used ? h : 0;
    if (row_bytes) *row_bytes = used ? (size_t)g.bps * w * (g.planar ? 1 : g.ch) : 0;
    return SRCNN_OK;
}

int srcnn_rgb_upscale_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                          const void* const src[4], const size_t src_pitch[4], void* const dst[4], const size_t dst_pitch[4],
                          void* dst_conv, size_t dst_conv_pitch, void* stream)
{
    RgbRule g;
    unsigned dw = 0, dh = 0;
    YuvPlane in[4], out[5], conv;
    int rc;
    if ((rc = rgb_rule_from_format(fmt, g))) return rc;
    if ((rc = check_rgb_args(g, w, h, multiply, filter, src, src_pitch, dst, dst_pitch, dst_conv, dst_conv_pitch, dw, dh, in, out, conv))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    TraceRange tr("srcnn rgb %ux%u -> %ux%u", w, h, dw, dh);
    return rgb_frame(sc.c, g, w, h, dw, dh, filter, in, out, conv);
}

// ---- one rectangle of an RGB(A) image (include/srcnn_amd_rgb_rect.h) ----
int srcnn_rgb_rect_abi_version(void) { return SRCNN_AMD_RGB_RECT_VERSION; }

int srcnn_rgb_rect_source(unsigned w, unsigned h, float multiply, int filter, unsigned x0, unsigned y0, unsigned rw, unsigned rh,
                          unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh)
{
    unsigned dw = 0, dh = 0, yx = 0, yy = 0, yw = 0, yh = 0, clx, chx, cly, chy;
    int rc;
    if (rw == 0 || rh == 0) return fail(SRCNN_E_ARG, "empty rect %ux%u", rw, rh);
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    if ((rc = check_rect_inside(dw, dh, x0, y0, rw, rh))) return rc;
    if ((rc = srcnn_y_path_rect_source(w, h, dw, dh, filter, x0, y0, rw, rh, &yx, &yy, &yw, &yh))) return rc;
    const int cfilter = chroma_filter(filter);
    axis_source_span(cfilter, dw, w, x0, x0 + rw, clx, chx);
    axis_source_span(cfilter, dh, h, y0, y0 + rh, cly, chy);
    const unsigned lx = std::min(yx, clx), ly = std::min(yy, cly);
    if (sx0) *sx0 = lx;
    if (sy0) *sy0 = ly;
    if (sw) *sw = std::max(yx + yw, chx) - lx;
    if (sh) *sh = std::max(yy + yh, chy) - ly;
    return SRCNN_OK;
}

int srcnn_rgb_upscale_rect_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                               const void* const src[4], const size_t src_pitch[4], unsigned x0, unsigned y0, unsigned rw,
                               unsigned rh, void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch,
                               void* stream)
{
    RgbRule g;
    unsigned dw = 0, dh = 0;
    YuvPlane in[4], out[5], conv;
    int rc;
    if ((rc = rgb_rule_from_format(fmt, g))) return rc;
    if ((rc = check_rgb_rect_args(g, w, h, multiply, filter, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, dst_conv, dst_conv_pitch,
                                  dw, dh, in, out, conv))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    return rgb_rect(sc.c, g, w, h, dw, dh, filter, in, out, conv, x0, y0, x0 + rw, y0 + rh);
}

// ---- one rectangle of a planar / semi-planar YUV frame (include/srcnn_amd_yuv_rect.h) ----
int srcnn_yuv_rect_abi_version(void) { return SRCNN_AMD_YUV_RECT_VERSION; }

int srcnn_yuv_rect_source(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter, unsigned x0, unsigned y0,
                          unsigned rw, unsigned rh, int plane, unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh)
{
    return yuv_rect_source(fmt, w, h, multiply, filter, x0, y0, rw, rh, plane, sx0, sy0, sw, sh);
}

int srcnn_yuv_upscale_rect_dev(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                               const void* const src[3], const size_t src_pitch[3], unsigned x0, unsigned y0, unsigned rw,
                               unsigned rh, void* const dst[3], const size_t dst_pitch[3], void* stream)
{
    YuvGeom g;
    unsigned dw = 0, dh = 0;
    YuvPlane in[3], out[3];
    int rc;
    if ((rc = yuv_geom_from_format(fmt, g))) return rc;
    if ((rc = check_yuv_rect_args(g, w, h, multiply, filter, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, dw, dh, in, out))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    return yuv_rect(sc.c, g, w, h, dw, dh, filter, in, out, x0, y0, x0 + rw, y0 + rh);
}

// ---- one rectangle of a packed YUV frame (include/srcnn_amd_yuv_packed_rect.h) ----
int srcnn_yuv_packed_rect_abi_version(void) { return SRCNN_AMD_YUV_PACKED_RECT_VERSION; }

int srcnn_yuv_packed_span_bytes(int format, unsigned width, unsigned x, unsigned n, unsigned* unit, size_t* byte_offset, size_t* bytes)
{
    return yuv_packed_span_bytes(format, width, x, n, unit, byte_offset, bytes);
}

int srcnn_yuv_packed_rect_source(int format, unsigned w, unsigned h, float multiply, int filter, unsigned x0, unsigned y0, unsigned rw,
                                 unsigned rh, unsigned* sx0, unsigned* sy0, unsigned* sw, unsigned* sh)
{
    return yuv_packed_rect_source(format, w, h, multiply, filter, x0, y0, rw, rh, sx0, sy0, sw, sh);
}

int srcnn_yuv_packed_upscale_rect_dev(int format, unsigned w, unsigned h, float multiply, int filter, const void* src, size_t src_pitch,
                                      unsigned x0, unsigned y0, unsigned rw, unsigned rh, void* dst, size_t dst_pitch, void* stream)
{
    YuvPackedGeom g;
    unsigned dw = 0, dh = 0;
    YuvPlane in, out;
    int rc;
    if ((rc = yuv_packed_geom(format, g))) return rc;
    if ((rc = check_yuv_packed_rect_args(g, w, h, multiply, filter, src, src_pitch, x0, y0, rw, rh, dst, dst_pitch, dw, dh, in, out))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    return yuv_packed_rect(sc.c, g, w, h, dw, dh, filter, in, out, x0, y0, x0 + rw, y0 + rh);
}

}  // extern "C"
