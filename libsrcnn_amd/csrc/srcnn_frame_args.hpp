// srcnn_frame_args.hpp -- the argument half of the frame calls (srcnn_frames.cpp): what a format comes down to, and everything
// srcnn_yuv420_upscale_dev, srcnn_yuv_upscale_dev, srcnn_yuv_packed_upscale_dev, srcnn_rgb_upscale_dev,
// srcnn_rgb_upscale_rect_dev, srcnn_yuv_upscale_rect_dev and srcnn_yuv_packed_upscale_rect_dev refuse before any device lookup.  It needs fail(), srcnn_output_size and the public headers only -- no HIP -- so tests/host/host_sanitize.cpp
// runs the pitch and end-of-plane pointer arithmetic under the CPU sanitizers.  Internal.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/srcnn_amd.h"
#include "../../include/srcnn_amd_rgb.h"
#include "../../include/srcnn_amd_yuv.h"
#include "../../include/srcnn_amd_yuv_ex.h"
#include "../../include/srcnn_amd_yuv_packed.h"
#include "srcnn_frame_rules.h"
#include "srcnn_y_path_geom.hpp"

namespace srcnn {

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// One pitched plane of a caller's frame.
struct YuvPlane {
    const unsigned char* lo = nullptr;   // first byte of the plane
    size_t pitch = 0, row_bytes = 0;
    unsigned rows = 0;
    const unsigned char* hi() const { return lo + pitch * (rows - 1) + row_bytes; }   // one past the last byte
};

inline bool overlaps(const YuvPlane& a, const YuvPlane& b) { return a.lo < b.hi() && b.lo < a.hi(); }

// What a planar / semi-planar format comes down to: plane count, chroma subsampling, sample width, read / write rule.
struct YuvGeom {
    bool semi = false;       // Y + interleaved UV (2 planes) instead of Y, U, V
    unsigned sx = 1, sy = 1; // chroma columns = ceil(w / 2^sx), rows = ceil(h / 2^sy)
    unsigned bps = 1;        // bytes per sample: 1 (depth 8) or 2
    Yuv16Rule rule;          // bps == 2
    unsigned ccols(unsigned w) const { return (w + sx) >> sx; }
    unsigned crows(unsigned h) const { return (h + sy) >> sy; }
};

// srcnn_yuv_format -> YuvGeom, or SRCNN_E_ARG
inline int yuv_geom_from_format(const srcnn_yuv_format* f, YuvGeom& g)
{
    if (!f) return fail(SRCNN_E_ARG, "NULL format");
    if (f->struct_size != sizeof(srcnn_yuv_format)) return fail(SRCNN_E_ARG, "struct_size %u is not %zu", f->struct_size, sizeof(srcnn_yuv_format));
    if (f->layout != SRCNN_YUV_PLANAR && f->layout != SRCNN_YUV_SEMIPLANAR) return fail(SRCNN_E_ARG, "unknown YUV layout %d", f->layout);
    if (f->chroma != SRCNN_YUV_420 && f->chroma != SRCNN_YUV_422 && f->chroma != SRCNN_YUV_444) return fail(SRCNN_E_ARG, "unknown chroma format %d", f->chroma);
    if (f->depth != 8 && f->depth != 10 && f->depth != 12 && f->depth != 14 && f->depth != 16) return fail(SRCNN_E_ARG, "unsupported depth %d", f->depth);
    if ((f->msb_aligned != 0 && f->msb_aligned != 1) || (f->depth == 8 && f->msb_aligned)) return fail(SRCNN_E_ARG, "bad msb_aligned %d at depth %d", f->msb_aligned, f->depth);
    g.semi = f->layout == SRCNN_YUV_SEMIPLANAR;
    g.sx = f->chroma == SRCNN_YUV_444 ? 0 : 1;
    g.sy = f->chroma == SRCNN_YUV_420 ? 1 : 0;
    g.bps = f->depth == 8 ? 1 : 2;
    if (g.bps == 2) {
        const unsigned s = (unsigned)f->depth - 8, shift = f->msb_aligned ? 16u - (unsigned)f->depth : 0u;
        g.rule.rshift = g.rule.lshift = shift;
        g.rule.mask = (1u << f->depth) - 1u;
        g.rule.up = (float)(1u << s);
        g.rule.down = 1.f / g.rule.up;
    }
    return SRCNN_OK;
}

// What a packed format comes down to: the kernels' rule, whether it carries alpha, the alignment of base and pitch.  Every
// packed format has one chroma row per luma row.
struct YuvPackedGeom {
    YuvPackedRule rule;
    bool alpha = false;
    unsigned align = 1;
    unsigned ccols(unsigned w) const { return yuv_packed_chroma_cols(rule.kind, w); }
    size_t row_bytes(unsigned w) const { return yuv_packed_row_bytes(rule.kind, w); }
};

// SRCNN_YUVP_* -> YuvPackedGeom, or SRCNN_E_ARG
inline int yuv_packed_geom(int format, YuvPackedGeom& g)
{
    // kind, depth of Y / U / V, depth of alpha (0: none), alignment, bit positions of (Y0 U Y1 V) or (Y U V A) in an 8-bit dword
    static const struct { int kind; unsigned depth, adepth, align, sh[4]; } T[] = {
        /* SRCNN_YUVP_YUY2 */ {kPk422x8, 8, 0, 1, {0, 8, 16, 24}},
        /* SRCNN_YUVP_UYVY */ {kPk422x8, 8, 0, 1, {8, 0, 24, 16}},
        /* SRCNN_YUVP_YVYU */ {kPk422x8, 8, 0, 1, {0, 24, 16, 8}},
        /* SRCNN_YUVP_Y210 */ {kPk422x16, 10, 0, 2, {0, 0, 0, 0}},
        /* SRCNN_YUVP_Y212 */ {kPk422x16, 12, 0, 2, {0, 0, 0, 0}},
        /* SRCNN_YUVP_Y216 */ {kPk422x16, 16, 0, 2, {0, 0, 0, 0}},
        /* SRCNN_YUVP_VUYA */ {kPk444x8, 8, 8, 1, {16, 8, 0, 24}},
        /* SRCNN_YUVP_Y410 */ {kPk410, 10, 2, 4, {0, 0, 0, 0}},
        /* SRCNN_YUVP_Y416 */ {kPk444x16, 16, 16, 2, {0, 0, 0, 0}},
        /* SRCNN_YUVP_V210 */ {kPkV210, 10, 0, 4, {0, 0, 0, 0}},
    };
    static_assert(SRCNN_YUVP_YUY2 == 0 && SRCNN_YUVP_V210 == 9 && sizeof(T) / sizeof(T[0]) == 10, "the table is indexed by SRCNN_YUVP_*");
    if (format < 0 || format > SRCNN_YUVP_V210) return fail(SRCNN_E_ARG, "unknown packed YUV format %d", format);
    const auto& t = T[format];
    g.rule.kind = t.kind;
    for (int k = 0; k < 4; ++k) g.rule.sh[k] = t.sh[k];
    g.rule.shift = t.kind == kPk422x16 ? 16u - t.depth : 0u;
    g.rule.mask = (1u << t.depth) - 1u;
    g.rule.amask = t.adepth ? (1u << t.adepth) - 1u : 0u;
    g.rule.up = (float)(1u << (t.depth - 8));
    g.rule.down = 1.f / g.rule.up;
    g.alpha = t.adepth != 0;
    g.align = t.align;
    return SRCNN_OK;
}

// srcnn_rgb_format -> RgbRule, or SRCNN_E_ARG
inline int rgb_rule_from_format(const srcnn_rgb_format* f, RgbRule& g)
{
    if (!f) return fail(SRCNN_E_ARG, "NULL format");
    if (f->struct_size != sizeof(srcnn_rgb_format)) return fail(SRCNN_E_ARG, "struct_size %u is not %zu", f->struct_size, sizeof(srcnn_rgb_format));
    if (f->layout != SRCNN_RGB_INTERLEAVED && f->layout != SRCNN_RGB_PLANAR) return fail(SRCNN_E_ARG, "unknown RGB layout %d", f->layout);
    if (f->order != SRCNN_RGB_ORDER_RGB && f->order != SRCNN_RGB_ORDER_BGR) return fail(SRCNN_E_ARG, "unknown channel order %d", f->order);
    if (f->alpha != 0 && f->alpha != 1) return fail(SRCNN_E_ARG, "bad alpha %d", f->alpha);
    if (f->depth != 8 && f->depth != 10 && f->depth != 12 && f->depth != 14 && f->depth != 16) return fail(SRCNN_E_ARG, "unsupported depth %d", f->depth);
    g.planar = f->layout == SRCNN_RGB_PLANAR;
    g.bgr = f->order == SRCNN_RGB_ORDER_BGR;
    g.ch = 3 + f->alpha;
    g.bps = f->depth == 8 ? 1 : 2;
    g.mask = (1u << f->depth) - 1u;
    g.up = (float)(1u << (f->depth - 8));
    g.down = 1.f / g.up;
    return SRCNN_OK;
}

// ---- the checks the three frame calls share ----

// Filter, size and scale of a frame call; sets the output size.  Every checker runs it straight after its own NULL-pointer
// checks (those, a bad filter and a zero size are all SRCNN_E_ARG).
inline int check_scale(unsigned w, unsigned h, float multiply, int filter, unsigned& dw, unsigned& dh)
{
    if (filter < 0 || filter > 4) return fail(SRCNN_E_ARG, "bad filter %d", filter);
    if (w == 0 || h == 0) return fail(SRCNN_E_ARG, "zero dimension %ux%u", w, h);
    if (!(multiply > 0.f) || !((float)w * multiply > 0.f) || !((float)h * multiply > 0.f)) return fail(SRCNN_E_SCALE, "multiply %g", multiply);
    // (the float products are truncated to unsigned below: keep them where that is defined, and inside the Y path's limits)
    if ((float)w * multiply >= 8388608.f || (float)h * multiply >= 1048577.f)
        return fail(SRCNN_E_UNSUPPORTED, "output of %ux%u x %g too large", w, h, multiply);
    if (srcnn_output_size(w, h, multiply, 0, &dw, &dh) != SRCNN_OK) return fail(SRCNN_E_SCALE, "scaled size of %ux%u x %g is zero", w, h, multiply);
    if (h > (1u << 20) || dh > kMaxGridRows || (unsigned long long)w * h > 0x7fffffffULL || (unsigned long long)dw * dh > 0x7fffffffULL)
        return fail(SRCNN_E_UNSUPPORTED, "%ux%u -> %ux%u is beyond the Y path's limits", w, h, dw, dh);
    return SRCNN_OK;
}

// Plane k of one side ("input", "output", "dst_conv") of a call: pitch 0 means tight rows; base and pitch are multiples of
// `align` (a power of two).
inline int describe_plane(YuvPlane& p, const void* base, size_t pitch, size_t row_bytes, unsigned rows, unsigned align,
                          const char* side, int k)
{
    p.lo = static_cast<const unsigned char*>(base);
    p.row_bytes = row_bytes;
    p.rows = rows;
    p.pitch = pitch ? pitch : row_bytes;
    if (p.pitch < p.row_bytes) return fail(SRCNN_E_ARG, "%s pitch %zu of plane %d is below its row of %zu bytes", side, p.pitch, k, p.row_bytes);
    if ((reinterpret_cast<uintptr_t>(p.lo) | p.pitch) & (align - 1))
        return fail(SRCNN_E_ARG, "%s plane %d: base address %p and pitch %zu must be multiples of %u", side, k, base, p.pitch, align);
    return SRCNN_OK;
}

inline int check_in_out_overlap(const YuvPlane* in, int nin, const YuvPlane* out, int nout)
{
    for (int a = 0; a < nin; ++a)
        for (int b = 0; b < nout; ++b)
            if (overlaps(in[a], out[b])) return fail(SRCNN_E_ARG, "input plane %d overlaps output plane %d", a, b);
    return SRCNN_OK;
}

inline int check_out_out_overlap(const YuvPlane* out, int nout)
{
    for (int a = 0; a < nout; ++a)
        for (int b = a + 1; b < nout; ++b)
            if (overlaps(out[a], out[b])) return fail(SRCNN_E_ARG, "output planes %d and %d overlap", a, b);
    return SRCNN_OK;
}

// ---- one checker per call: everything it refuses beyond the format itself ----

// (Output planes that overlap each other are not refused by the two YUV checkers, only by the RGB one: that is what the calls
// have always accepted, and changing it is a change to the interface.)
inline int check_yuv_args(const YuvGeom& g, unsigned w, unsigned h, float multiply, int filter, const void* const src[3],
                          const size_t src_pitch[3], void* const dst[3], const size_t dst_pitch[3], unsigned& dw,
                          unsigned& dh, YuvPlane in[3], YuvPlane out[3])
{
    const int np = g.semi ? 2 : 3;
    if (!src || !dst) return fail(SRCNN_E_ARG, "NULL plane array");
    for (int k = 0; k < np; ++k)
        if (!src[k] || !dst[k]) return fail(SRCNN_E_ARG, "NULL plane %d", k);
    int rc;
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    for (int side = 0; side < 2; ++side) {
        const unsigned pw = side ? dw : w, ph = side ? dh : h, pcw = g.ccols(pw), pch = g.crows(ph);
        const size_t* pitch = side ? dst_pitch : src_pitch;
        for (int k = 0; k < np; ++k) {
            const size_t row_bytes = (size_t)g.bps * (k == 0 ? pw : (g.semi ? 2 * (size_t)pcw : pcw));
            if ((rc = describe_plane((side ? out : in)[k], side ? dst[k] : src[k], pitch ? pitch[k] : 0, row_bytes, k == 0 ? ph : pch,
                                     g.bps, side ? "output" : "input", k))) return rc;
        }
    }
    return check_in_out_overlap(in, np, out, np);
}

inline int check_yuv_packed_args(const YuvPackedGeom& g, unsigned w, unsigned h, float multiply, int filter, const void* src,
                                 size_t src_pitch, void* dst, size_t dst_pitch, unsigned& dw, unsigned& dh, YuvPlane& in, YuvPlane& out)
{
    if (!src || !dst) return fail(SRCNN_E_ARG, "NULL frame");
    int rc;
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    if ((rc = describe_plane(in, src, src_pitch, g.row_bytes(w), h, g.align, "input", 0))) return rc;
    if ((rc = describe_plane(out, dst, dst_pitch, g.row_bytes(dw), dh, g.align, "output", 0))) return rc;
    return check_in_out_overlap(&in, 1, &out, 1);
}

// The planes of an RGB(A) call, both sides: the w x h source image, a destination of ow x oh pixels (and dst_conv of that size),
// then the overlap rules.  out[] has room for the planes and dst_conv; conv.lo stays NULL when the caller asks for no
// truncated Y' plane.
inline int describe_rgb_planes(const RgbRule& g, unsigned w, unsigned h, unsigned ow, unsigned oh, const void* const src[4],
                               const size_t src_pitch[4], void* const dst[4], const size_t dst_pitch[4], void* dst_conv,
                               size_t dst_conv_pitch, YuvPlane in[4], YuvPlane out[5], YuvPlane& conv)
{
    const int np = g.planar ? g.ch : 1;
    int rc;
    const size_t spp = g.planar ? 1 : (size_t)g.ch;                 // samples per pixel of one plane
    for (int k = 0; k < np; ++k) {
        if ((rc = describe_plane(in[k], src[k], src_pitch ? src_pitch[k] : 0, (size_t)g.bps * spp * w, h, g.bps, "input", k))) return rc;
        if ((rc = describe_plane(out[k], dst[k], dst_pitch ? dst_pitch[k] : 0, (size_t)g.bps * spp * ow, oh, g.bps, "output", k))) return rc;
    }
    int nout = np;
    if (dst_conv) {
        if ((rc = describe_plane(conv, dst_conv, dst_conv_pitch, (size_t)g.bps * ow, oh, g.bps, "dst_conv", 0))) return rc;
        out[nout++] = conv;
    }
    if ((rc = check_in_out_overlap(in, np, out, nout))) return rc;
    return check_out_out_overlap(out, nout);
}

inline int check_rgb_planes_given(const RgbRule& g, const void* const src[4], void* const dst[4])
{
    if (!src || !dst) return fail(SRCNN_E_ARG, "NULL plane array");
    for (int k = 0; k < (g.planar ? g.ch : 1); ++k)
        if (!src[k] || !dst[k]) return fail(SRCNN_E_ARG, "NULL plane %d", k);
    return SRCNN_OK;
}

inline int check_rgb_args(const RgbRule& g, unsigned w, unsigned h, float multiply, int filter, const void* const src[4],
                          const size_t src_pitch[4], void* const dst[4], const size_t dst_pitch[4], void* dst_conv,
                          size_t dst_conv_pitch, unsigned& dw, unsigned& dh, YuvPlane in[4], YuvPlane out[5], YuvPlane& conv)
{
    int rc;
    if ((rc = check_rgb_planes_given(g, src, dst))) return rc;
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    return describe_rgb_planes(g, w, h, dw, dh, src, src_pitch, dst, dst_pitch, dst_conv, dst_conv_pitch, in, out, conv);
}

// A rect [x0, x0 + rw) x [y0, y0 + rh) of a dw x dh output: not empty, inside (the sums taken in 64 bits)
inline int check_rect_inside(unsigned dw, unsigned dh, unsigned x0, unsigned y0, unsigned rw, unsigned rh)
{
    if (rw == 0 || rh == 0) return fail(SRCNN_E_ARG, "empty rect %ux%u", rw, rh);
    if ((unsigned long long)x0 + rw > dw || (unsigned long long)y0 + rh > dh)
        return fail(SRCNN_E_ARG, "rect %ux%u at (%u,%u) is not inside the %ux%u output", rw, rh, x0, y0, dw, dh);
    return SRCNN_OK;
}

// srcnn_rgb_upscale_rect_dev: the rules of check_rgb_args, with a destination (and dst_conv) of rw x rh pixels.
inline int check_rgb_rect_args(const RgbRule& g, unsigned w, unsigned h, float multiply, int filter, const void* const src[4],
                               const size_t src_pitch[4], unsigned x0, unsigned y0, unsigned rw, unsigned rh, void* const dst[4],
                               const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch, unsigned& dw, unsigned& dh,
                               YuvPlane in[4], YuvPlane out[5], YuvPlane& conv)
{
    int rc;
    if ((rc = check_rgb_planes_given(g, src, dst))) return rc;
    if (rw == 0 || rh == 0) return fail(SRCNN_E_ARG, "empty rect %ux%u", rw, rh);
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    if ((rc = check_rect_inside(dw, dh, x0, y0, rw, rh))) return rc;
    return describe_rgb_planes(g, w, h, rw, rh, src, src_pitch, dst, dst_pitch, dst_conv, dst_conv_pitch, in, out, conv);
}

// The chroma samples that cover luma rect [x0, x1) x [y0, y1): [cx0, cx1) x [cy0, cy1) on the chroma grid.  x0 (y0) is even
// where the format subsamples that axis, so these are the chroma planes of an (x1 - x0) x (y1 - y0) frame.
struct YuvChromaRect {
    unsigned cx0, cy0, cx1, cy1;
    YuvChromaRect(const YuvGeom& g, unsigned x0, unsigned y0, unsigned x1, unsigned y1)
        : cx0(x0 >> g.sx), cy0(y0 >> g.sy), cx1(g.ccols(x1)), cy1(g.crows(y1)) {}
};

// A rect origin the chroma grid cannot express: odd x0 under horizontal subsampling, odd y0 under vertical
inline int check_yuv_rect_origin(const YuvGeom& g, unsigned x0, unsigned y0)
{
    if ((g.sx && (x0 & 1)) || (g.sy && (y0 & 1)))
        return fail(SRCNN_E_ARG, "rect origin (%u,%u) must be even where the format subsamples chroma (columns: %s, rows: %s)", x0, y0,
                    g.sx ? "yes" : "no", g.sy ? "yes" : "no");
    return SRCNN_OK;
}

// srcnn_yuv_upscale_rect_dev: the rules of check_yuv_args with the WHOLE w x h frame as the source and the planes of an rw x rh
// frame as the destination, the rect's own rules between the scale and the planes, and -- unlike the whole-frame calls --
// destination planes that overlap each other refused (a rect is repainted inside a shared surface: a slip shows here first).
// It comes in a frame half and a per-rect half, which the YUV rect LIST call (srcnn_yuv_rect_list_call.cpp) runs once and once
// per item: describe_yuv_side for the source, then check_yuv_rect_place and check_yuv_rect_planes for every rect.

// One side ("input" / "output") of a planar / semi-planar call: the planes of a pw x ph frame in g
inline int describe_yuv_side(const YuvGeom& g, unsigned pw, unsigned ph, const void* const base[3], const size_t pitch[3], const char* side,
                             YuvPlane p[3])
{
    const unsigned pcw = g.ccols(pw), pch = g.crows(ph);
    int rc;
    for (int k = 0; k < (g.semi ? 2 : 3); ++k) {
        const size_t row_bytes = (size_t)g.bps * (k == 0 ? pw : (g.semi ? 2 * (size_t)pcw : pcw));
        if ((rc = describe_plane(p[k], base[k], pitch ? pitch[k] : 0, row_bytes, k == 0 ? ph : pch, g.bps, side, k))) return rc;
    }
    return SRCNN_OK;
}

// per rect, geometry: not empty, inside dw x dh, an origin the chroma grid can express
inline int check_yuv_rect_place(const YuvGeom& g, unsigned dw, unsigned dh, unsigned x0, unsigned y0, unsigned rw, unsigned rh)
{
    int rc;
    if ((rc = check_rect_inside(dw, dh, x0, y0, rw, rh))) return rc;
    return check_yuv_rect_origin(g, x0, y0);
}

// per rect, memory: the planes of an rw x rh frame as the destination, against the source planes `in` and each other
inline int check_yuv_rect_planes(const YuvGeom& g, unsigned rw, unsigned rh, void* const dst[3], const size_t dst_pitch[3], const YuvPlane in[3],
                                 YuvPlane out[3])
{
    const int np = g.semi ? 2 : 3;
    int rc;
    if ((rc = describe_yuv_side(g, rw, rh, dst, dst_pitch, "output", out))) return rc;
    if ((rc = check_in_out_overlap(in, np, out, np))) return rc;
    return check_out_out_overlap(out, np);
}

inline int check_yuv_rect_args(const YuvGeom& g, unsigned w, unsigned h, float multiply, int filter, const void* const src[3],
                               const size_t src_pitch[3], unsigned x0, unsigned y0, unsigned rw, unsigned rh, void* const dst[3],
                               const size_t dst_pitch[3], unsigned& dw, unsigned& dh, YuvPlane in[3], YuvPlane out[3])
{
    const int np = g.semi ? 2 : 3;
    if (!src || !dst) return fail(SRCNN_E_ARG, "NULL plane array");
    for (int k = 0; k < np; ++k)
        if (!src[k] || !dst[k]) return fail(SRCNN_E_ARG, "NULL plane %d", k);
    if (rw == 0 || rh == 0) return fail(SRCNN_E_ARG, "empty rect %ux%u", rw, rh);
    int rc;
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    if ((rc = check_yuv_rect_place(g, dw, dh, x0, y0, rw, rh))) return rc;
    if ((rc = describe_yuv_side(g, w, h, src, src_pitch, "input", in))) return rc;
    return check_yuv_rect_planes(g, rw, rh, dst, dst_pitch, in, out);
}

// The unit rule of a packed span (include/srcnn_amd_yuv_packed_rect.h): pixels [x, x + n) of a `width`-pixel row, already known
// to lie inside it.  x is a multiple of the unit; n is one, or the span ends at the row's end.  A packing unit cannot be
// half-written without reading the destination.
inline int check_yuv_packed_unit(const YuvPackedGeom& g, unsigned width, unsigned x, unsigned n)
{
    const unsigned unit = yuv_packed_unit(g.rule.kind);
    if (x % unit || (n % unit && x + n != width))
        return fail(SRCNN_E_ARG, "pixels [%u, %u + %u) of a %u-pixel row: the first must be a multiple of %u, and the count as well unless they end the row",
                    x, x, n, width, unit);
    return SRCNN_OK;
}

// srcnn_yuv_packed_upscale_rect_dev: the rules of check_yuv_packed_args with the WHOLE w x h frame as the source and rh row
// segments of the rect's span as the destination, the rect's own rules between the scale and the planes.  It comes in a frame
// half and a per-rect half, which the packed rect LIST call (srcnn_yuv_packed_rect_list_call.cpp) runs once and once per item:
// describe_yuv_packed_source for the frame, then check_yuv_packed_rect_place and check_yuv_packed_rect_dst for every rect.

// the frame: the WHOLE w x h packed source
inline int describe_yuv_packed_source(const YuvPackedGeom& g, unsigned w, unsigned h, const void* src, size_t src_pitch, YuvPlane& in)
{
    return describe_plane(in, src, src_pitch, g.row_bytes(w), h, g.align, "input", 0);
}

// per rect, geometry: not empty, inside dw x dh, under the unit rule
inline int check_yuv_packed_rect_place(const YuvPackedGeom& g, unsigned dw, unsigned dh, unsigned x0, unsigned y0, unsigned rw, unsigned rh)
{
    int rc;
    if ((rc = check_rect_inside(dw, dh, x0, y0, rw, rh))) return rc;
    return check_yuv_packed_unit(g, dw, x0, rw);
}

// per rect, memory: rh row segments of the rect's span as the destination, against the source `in`
inline int check_yuv_packed_rect_dst(const YuvPackedGeom& g, unsigned dw, unsigned x0, unsigned rw, unsigned rh, void* dst, size_t dst_pitch,
                                     const YuvPlane& in, YuvPlane& out)
{
    int rc;
    size_t off = 0, n = 0;
    yuv_packed_span(g.rule.kind, dw, x0, rw, off, n);
    if ((rc = describe_plane(out, dst, dst_pitch, n, rh, g.align, "output", 0))) return rc;
    return check_in_out_overlap(&in, 1, &out, 1);
}

inline int check_yuv_packed_rect_args(const YuvPackedGeom& g, unsigned w, unsigned h, float multiply, int filter, const void* src,
                                      size_t src_pitch, unsigned x0, unsigned y0, unsigned rw, unsigned rh, void* dst, size_t dst_pitch,
                                      unsigned& dw, unsigned& dh, YuvPlane& in, YuvPlane& out)
{
    if (!src || !dst) return fail(SRCNN_E_ARG, "NULL frame");
    if (rw == 0 || rh == 0) return fail(SRCNN_E_ARG, "empty rect %ux%u", rw, rh);
    int rc;
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    if ((rc = check_yuv_packed_rect_place(g, dw, dh, x0, y0, rw, rh))) return rc;
    if ((rc = describe_yuv_packed_source(g, w, h, src, src_pitch, in))) return rc;
    return check_yuv_packed_rect_dst(g, dw, x0, rw, rh, dst, dst_pitch, in, out);
}

}  // namespace srcnn
