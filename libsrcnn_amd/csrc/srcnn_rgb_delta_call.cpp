// srcnn_rgb_delta_call.cpp -- the RGB(A) delta call (include/srcnn_amd_rgb_delta.h): its argument checks and the RGB(A) image as
// a surface of the skeleton in srcnn_delta_call.hpp -- the RGB(A) span tables, the launch of k_delta_flags_bytes
// (srcnn_delta.hip) and the repaint.  Nothing of the list call, the rect call or their kernels is changed: the rects go through
// the public srcnn_rgb_upscale_rect_list_dev.
#include <vector>

#include "../../include/srcnn_amd_rgb_delta.h"
#include "srcnn_delta.h"
#include "srcnn_delta_call.hpp"
#include "srcnn_frame_args.hpp"
#include "srcnn_rgb_delta.hpp"

using namespace srcnn;

namespace {

// Two RGB(A) images over one grid and the destination of the whole operation.  check_geometry fills format, geometry and scale,
// tile and grid -- what every entry point refuses first, in this order -- check_sources and describe_destination the planes.
struct RgbSurface {
    static constexpr DeltaSpanOwner kOwner = DeltaSpanOwner::Rgb;
    static constexpr const char *kTrace = "rgb delta", *kName = "rgb_upscale_delta", *kEntry = "srcnn_rgb_upscale_delta_dev";
    RgbRule g;
    RgbListLayout lay;
    const srcnn_rgb_format* fmt = nullptr;
    unsigned w = 0, h = 0, dw = 0, dh = 0;
    float multiply = 0;
    int filter = 0, np = 1;
    DeltaGrid grid;
    const void* const* cur = nullptr;                // as the caller gave them
    const size_t* cur_pitch = nullptr;
    bool prev = false;
    YuvPlane in_prev[4], in_cur[4];
    RgbDeltaDst d;

    bool has_prev() const { return prev; }
    // rgb_delta_axis_spans: the Y path's span united with the chroma taps'
    int spans(Call& c, std::vector<DeltaSpan>& xs, std::vector<DeltaSpan>& ys) const
    {
        int rc;
        const int cfilter = chroma_filter(filter);
        TableRef th, tv, cth, ctv;
        if (dw != w && ((rc = get_table(c, filter, dw, w, th)) || (rc = get_table(c, cfilter, dw, w, cth)))) return rc;
        if (dh != h && ((rc = get_table(c, filter, dh, h, tv)) || (rc = get_table(c, cfilter, dh, h, ctv)))) return rc;
        rgb_delta_axis_spans(th ? th->h_first.data() : nullptr, th ? th->h_taps.data() : nullptr, cth ? cth->h_first.data() : nullptr,
                             cth ? cth->h_taps.data() : nullptr, dw, w, grid.tile_w, xs);
        rgb_delta_axis_spans(tv ? tv->h_first.data() : nullptr, tv ? tv->h_taps.data() : nullptr, ctv ? ctv->h_first.data() : nullptr,
                             ctv ? ctv->h_taps.data() : nullptr, dh, h, grid.tile_h, ys);
        return SRCNN_OK;
    }
    int queue_flags(Call& c, unsigned char* d_flags) const
    {
        DeltaBytePlanes p{};
        p.planes = (unsigned)np;
        p.row_bytes = (unsigned)lay.row_bytes(w);
        p.rows = h;
        p.bpp = (unsigned)lay.row_bytes(1);
        for (int k = 0; k < np; ++k) {
            p.prev[k] = in_prev[k].lo; p.prev_pitch[k] = in_prev[k].pitch;
            p.cur[k] = in_cur[k].lo; p.cur_pitch[k] = in_cur[k].pitch;
        }
        launch_delta_flags_bytes(p, c.ws->delta_spans.data(), grid.cols, grid.rows, d_flags, c.s);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail(SRCNN_E_HIP, "rgb_delta_flags: %s", hipGetErrorString(e));
        return SRCNN_OK;
    }
    int repaint(const std::vector<DeltaRect>& rects, void* stream) const
    {
        std::vector<srcnn_rgb_rect_item> items(rects.size());
        rgb_delta_items(rects, lay, d, items.data(), items.size());
        return srcnn_rgb_upscale_rect_list_dev(fmt, w, h, multiply, filter, cur, cur_pitch, items.data(), (unsigned)items.size(),
                                               (unsigned)sizeof(srcnn_rgb_rect_item), stream);
    }
};

int rgb_layout(const srcnn_rgb_format* fmt, RgbSurface& a)
{
    if (const int rc = rgb_rule_from_format(fmt, a.g)) return rc;
    a.fmt = fmt;
    a.lay = RgbListLayout{a.g.bps, (unsigned)a.g.ch, a.g.planar};
    a.np = (int)a.lay.planes();
    return SRCNN_OK;
}

int check_geometry(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter, unsigned tile_w, unsigned tile_h, RgbSurface& a)
{
    int rc;
    if ((rc = rgb_layout(fmt, a))) return rc;
    a.w = w; a.h = h; a.multiply = multiply; a.filter = filter;
    if ((rc = check_scale(w, h, multiply, filter, a.dw, a.dh))) return rc;
    // (a row's bytes fit 32 bits with room to spare: h * multiply >= 1 and w * multiply < 2^23 give w < 2^23 h, and with
    // w h < 2^31 that is w < 2^27 -- a row of at most 8 w < 2^30 bytes)
    return delta_grid(w, h, a.dw, a.dh, filter, tile_w, tile_h, a.grid);
}

// the planes of both source images, under the rules of include/srcnn_amd_rgb.h; prev == NULL: no previous image
int check_sources(RgbSurface& a, const void* const prev[4], const size_t prev_pitch[4], const void* const cur[4], const size_t cur_pitch[4])
{
    int rc;
    if (!cur) return fail(SRCNN_E_ARG, "NULL plane array of the current image");
    for (int k = 0; k < a.np; ++k)
        if ((prev && !prev[k]) || !cur[k]) return fail(SRCNN_E_ARG, "NULL plane %d", k);
    for (int k = 0; prev && k < a.np; ++k)
        if ((rc = describe_plane(a.in_prev[k], prev[k], prev_pitch ? prev_pitch[k] : 0, a.lay.row_bytes(a.w), a.h, a.g.bps, "previous", k))) return rc;
    for (int k = 0; k < a.np; ++k)
        if ((rc = describe_plane(a.in_cur[k], cur[k], cur_pitch ? cur_pitch[k] : 0, a.lay.row_bytes(a.w), a.h, a.g.bps, "current", k))) return rc;
    a.prev = prev != nullptr;
    a.cur = cur;
    a.cur_pitch = cur_pitch;
    return SRCNN_OK;
}

// dst (and dst_conv) as a dw x dh image in the format: planes in out[0 .. nout), pitches resolved in a.d
int describe_destination(RgbSurface& a, void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch, YuvPlane out[5], int& nout)
{
    int rc;
    RgbDeltaDst& d = a.d;
    d = RgbDeltaDst{};
    nout = 0;
    for (int k = 0; dst && k < a.np; ++k) {
        if (!dst[k]) return fail(SRCNN_E_ARG, "NULL plane %d", k);
        if ((rc = describe_plane(out[k], dst[k], dst_pitch ? dst_pitch[k] : 0, a.lay.row_bytes(a.dw), a.dh, a.g.bps, "output", k))) return rc;
        d.plane[k] = dst[k];
        d.pitch[k] = out[k].pitch;
        nout = k + 1;
    }
    if (!dst)                                        // (srcnn_rgb_delta_rects: NULL destinations, the pitches still resolved)
        for (int k = 0; k < a.np; ++k) d.pitch[k] = dst_pitch && dst_pitch[k] ? dst_pitch[k] : a.lay.row_bytes(a.dw);
    if (dst_conv) {
        if ((rc = describe_plane(out[nout], dst_conv, dst_conv_pitch, (size_t)a.g.bps * a.dw, a.dh, a.g.bps, "dst_conv", 0))) return rc;
        d.conv = dst_conv;
        d.conv_pitch = out[nout].pitch;
        ++nout;
    }
    return SRCNN_OK;
}

}  // namespace

extern "C" {

int srcnn_rgb_delta_abi_version(void) { return SRCNN_AMD_RGB_DELTA_VERSION; }

int srcnn_rgb_delta_grid(unsigned w, unsigned h, float multiply, int filter, unsigned tile_w, unsigned tile_h, unsigned* dw, unsigned* dh,
                         unsigned* cols, unsigned* rows)
{
    unsigned ow = 0, oh = 0;
    DeltaGrid g;
    int rc;
    if ((rc = check_scale(w, h, multiply, filter, ow, oh))) return rc;
    if ((rc = delta_grid(w, h, ow, oh, filter, tile_w, tile_h, g))) return rc;
    if (dw) *dw = ow;
    if (dh) *dh = oh;
    if (cols) *cols = g.cols;
    if (rows) *rows = g.rows;
    return SRCNN_OK;
}

int srcnn_rgb_delta_flags_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter, const void* const prev[4],
                              const size_t prev_pitch[4], const void* const cur[4], const size_t cur_pitch[4], unsigned tile_w,
                              unsigned tile_h, unsigned char* d_flags, void* stream)
{
    int rc;
    RgbSurface a;
    if ((rc = check_geometry(fmt, w, h, multiply, filter, tile_w, tile_h, a))) return rc;
    if (!d_flags) return fail(SRCNN_E_ARG, "NULL d_flags");
    if ((rc = check_sources(a, prev, prev_pitch, cur, cur_pitch))) return rc;
    return delta_flags_call(a, d_flags, stream);
}

int srcnn_rgb_delta_rects(const unsigned char* flags, unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h, const srcnn_rgb_format* fmt,
                          unsigned dw, unsigned dh, void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch,
                          srcnn_rgb_rect_item* items, unsigned cap, unsigned item_size, unsigned* n)
{
    int rc;
    if (!n) return fail(SRCNN_E_ARG, "NULL n");
    *n = 0;
    RgbSurface a;
    if ((rc = rgb_layout(fmt, a))) return rc;
    a.dw = dw;
    a.dh = dh;
    if ((rc = check_delta_tiles(cols, rows, tile_w, tile_h, dw, dh))) return rc;
    if (!flags) return fail(SRCNN_E_ARG, "NULL flags");
    if (item_size != sizeof(srcnn_rgb_rect_item)) return fail(SRCNN_E_ARG, "item_size %u is not sizeof(srcnn_rgb_rect_item) = %zu", item_size, sizeof(srcnn_rgb_rect_item));
    if (!items && cap) return fail(SRCNN_E_ARG, "NULL items with cap = %u", cap);
    YuvPlane out[5];
    int nout = 0;
    if ((rc = describe_destination(a, dst, dst_pitch, dst_conv, dst_conv_pitch, out, nout))) return rc;
    std::vector<DeltaRect> rects;
    *n = delta_coalesce(flags, cols, rows, tile_w, tile_h, dw, dh, rects);
    if (!items && cap == 0) return SRCNN_OK;         // counts only
    if (!rgb_delta_items(rects, a.lay, a.d, items, cap)) return fail(SRCNN_E_ARG, "%u rects do not fit %u items", *n, cap);
    return SRCNN_OK;
}

int srcnn_rgb_upscale_delta_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter, const void* const prev[4],
                                const size_t prev_pitch[4], const void* const cur[4], const size_t cur_pitch[4], unsigned tile_w,
                                unsigned tile_h, void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch,
                                void* stream, srcnn_delta_stats* stats)
{
    int rc, nout = 0;
    RgbSurface a;
    YuvPlane out[5];
    if ((rc = check_geometry(fmt, w, h, multiply, filter, tile_w, tile_h, a))) return rc;
    if ((rc = check_delta_stats(stats))) return rc;
    if ((rc = check_sources(a, prev, prev_pitch, cur, cur_pitch))) return rc;
    if (!dst) return fail(SRCNN_E_ARG, "NULL plane array of the destination");
    if ((rc = describe_destination(a, dst, dst_pitch, dst_conv, dst_conv_pitch, out, nout))) return rc;
    if (prev && (rc = check_in_out_overlap(a.in_prev, a.np, out, nout))) return rc;
    if ((rc = check_in_out_overlap(a.in_cur, a.np, out, nout))) return rc;
    if ((rc = check_out_out_overlap(out, nout))) return rc;
    return delta_call(a, stream, stats);
}

}  // extern "C"
