// srcnn_rgb_delta_call.cpp -- the RGB(A) delta call (include/srcnn_amd_rgb_delta.h), modelled on srcnn_delta_call.cpp: its
// argument checks, the RGB(A) span tables of a stream's workspace, the launch of k_delta_flags_bytes (srcnn_delta.hip) and, for
// the whole operation, the one wait for the flags, the coalescer and the whole-frame rule of srcnn_delta.hpp, and the RGB(A) rect
// list call that repaints.  Nothing of the list call, the rect call or their kernels is changed: the rects go through the public
// srcnn_rgb_upscale_rect_list_dev.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/srcnn_amd_rgb_delta.h"
#include "srcnn_delta.h"
#include "srcnn_frame_args.hpp"
#include "srcnn_rect_list_call.hpp"
#include "srcnn_rgb_delta.hpp"

using namespace srcnn;

namespace {

// format, geometry and scale, tile and grid: what every entry point refuses first, in this order
struct Geometry {
    RgbRule g;
    RgbListLayout lay;
    unsigned dw = 0, dh = 0;
    DeltaGrid grid;
    int np = 1;
    size_t tiles() const { return (size_t)grid.cols * grid.rows; }
};

int check_geometry(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter, unsigned tile_w, unsigned tile_h, Geometry& a)
{
    int rc;
    if ((rc = rgb_rule_from_format(fmt, a.g))) return rc;
    a.lay = RgbListLayout{a.g.bps, (unsigned)a.g.ch, a.g.planar};
    a.np = (int)a.lay.planes();
    if ((rc = check_scale(w, h, multiply, filter, a.dw, a.dh))) return rc;
    // (a row's bytes fit 32 bits with room to spare: h * multiply >= 1 and w * multiply < 2^23 give w < 2^23 h, and with
    // w h < 2^31 that is w < 2^27 -- a row of at most 8 w < 2^30 bytes)
    return delta_grid(w, h, a.dw, a.dh, filter, tile_w, tile_h, a.grid);
}

// the planes of both source images, under the rules of include/srcnn_amd_rgb.h; prev == NULL: no previous image
int check_sources(const Geometry& a, unsigned w, unsigned h, const void* const prev[4], const size_t prev_pitch[4], const void* const cur[4],
                  const size_t cur_pitch[4], YuvPlane in_prev[4], YuvPlane in_cur[4])
{
    int rc;
    if (!cur) return fail(SRCNN_E_ARG, "NULL plane array of the current image");
    for (int k = 0; k < a.np; ++k)
        if ((prev && !prev[k]) || !cur[k]) return fail(SRCNN_E_ARG, "NULL plane %d", k);
    for (int k = 0; prev && k < a.np; ++k)
        if ((rc = describe_plane(in_prev[k], prev[k], prev_pitch ? prev_pitch[k] : 0, a.lay.row_bytes(w), h, a.g.bps, "previous", k))) return rc;
    for (int k = 0; k < a.np; ++k)
        if ((rc = describe_plane(in_cur[k], cur[k], cur_pitch ? cur_pitch[k] : 0, a.lay.row_bytes(w), h, a.g.bps, "current", k))) return rc;
    return SRCNN_OK;
}

// dst (and dst_conv) as a dw x dh image in the format: planes in out[0 .. nout), pitches resolved in d
int describe_destination(const Geometry& a, void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch, YuvPlane out[5],
                         int& nout, RgbDeltaDst& d)
{
    int rc;
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

// The RGB(A) span tables of this geometry in the workspace (rgb_delta_axis_spans: the Y path's span united with the chroma taps'),
// uploaded when the geometry changes, as the Y call's ensure_spans does it.  The eighth word of the key says whose tables they
// are: the two calls' tables differ for one geometry and share DeltaStage, so they must not answer for each other.
constexpr unsigned kRgbSpans = 1;      // (the Y call's key ends in 0)
int ensure_spans(Call& c, unsigned w, unsigned h, int filter, const Geometry& a)
{
    Workspace& ws = *c.ws;
    DeltaStage& st = ws.delta_stage;
    const unsigned dw = a.dw, dh = a.dh;
    const DeltaGrid& g = a.grid;
    const unsigned key[8] = {w, h, dw, dh, (unsigned)filter, g.tile_w, g.tile_h, kRgbSpans};
    const size_t words = delta_span_words(g.cols, g.rows);
    if (st.valid && !memcmp(st.key, key, sizeof key) && ws.delta_spans.size() >= words) return SRCNN_OK;
    if (foreign_capture(c))
        return fail(SRCNN_E_UNSUPPORTED, "the span tables of %ux%u -> %ux%u are not on the device yet, and the stream is being captured: run the call once outside the capture", w, h, dw, dh);
    int rc;
    const int cfilter = chroma_filter(filter);
    std::vector<DeltaSpan> xs, ys;
    TableRef th, tv, cth, ctv;
    if (dw != w && ((rc = get_table(c, filter, dw, w, th)) || (rc = get_table(c, cfilter, dw, w, cth)))) return rc;
    if (dh != h && ((rc = get_table(c, filter, dh, h, tv)) || (rc = get_table(c, cfilter, dh, h, ctv)))) return rc;
    rgb_delta_axis_spans(th ? th->h_first.data() : nullptr, th ? th->h_taps.data() : nullptr, cth ? cth->h_first.data() : nullptr,
                         cth ? cth->h_taps.data() : nullptr, dw, w, g.tile_w, xs);
    rgb_delta_axis_spans(tv ? tv->h_first.data() : nullptr, tv ? tv->h_taps.data() : nullptr, ctv ? ctv->h_first.data() : nullptr,
                         ctv ? ctv->h_taps.data() : nullptr, dh, h, g.tile_h, ys);
    if (!delta_spans_monotone(xs, w) || !delta_spans_monotone(ys, h))
        return fail(SRCNN_E_UNSUPPORTED, "the tile spans of %ux%u -> %ux%u (filter %d) are not monotone", w, h, dw, dh, filter);
    std::vector<unsigned> image(words);
    delta_span_image(xs, ys, image.data());
    st.valid = false;
    if ((rc = ws.grow(ws.delta_spans, words))) return rc;
    if ((rc = copy_h2d_any(*c.cx, ws.delta_spans.data(), image.data(), sizeof(unsigned) * words, c.s))) return rc;
    memcpy(st.key, key, sizeof key);
    st.valid = true;
    return SRCNN_OK;
}

int queue_flags(Call& c, const Geometry& a, unsigned w, unsigned h, const YuvPlane prev[4], const YuvPlane cur[4], unsigned char* d_flags)
{
    DeltaBytePlanes p{};
    p.planes = (unsigned)a.np;
    p.row_bytes = (unsigned)a.lay.row_bytes(w);
    p.rows = h;
    p.bpp = (unsigned)a.lay.row_bytes(1);
    for (int k = 0; k < a.np; ++k) {
        p.prev[k] = prev[k].lo; p.prev_pitch[k] = prev[k].pitch;
        p.cur[k] = cur[k].lo; p.cur_pitch[k] = cur[k].pitch;
    }
    launch_delta_flags_bytes(p, c.ws->delta_spans.data(), a.grid.cols, a.grid.rows, d_flags, c.s);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail(SRCNN_E_HIP, "rgb_delta_flags: %s", hipGetErrorString(e));
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
    Geometry a;
    YuvPlane in_prev[4], in_cur[4];
    if ((rc = check_geometry(fmt, w, h, multiply, filter, tile_w, tile_h, a))) return rc;
    if (!d_flags) return fail(SRCNN_E_ARG, "NULL d_flags");
    if ((rc = check_sources(a, w, h, prev, prev_pitch, cur, cur_pitch, in_prev, in_cur))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    Call& c = sc.c;
    if (!prev) {                                     // no previous image: everything is dirty
        HIP_TRY(hipMemsetAsync(d_flags, 1, a.tiles(), c.s));
        return SRCNN_OK;
    }
    if ((rc = ensure_spans(c, w, h, filter, a))) return rc;
    return queue_flags(c, a, w, h, in_prev, in_cur, d_flags);
}

int srcnn_rgb_delta_rects(const unsigned char* flags, unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h, const srcnn_rgb_format* fmt,
                          unsigned dw, unsigned dh, void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch,
                          srcnn_rgb_rect_item* items, unsigned cap, unsigned item_size, unsigned* n)
{
    int rc;
    if (!n) return fail(SRCNN_E_ARG, "NULL n");
    *n = 0;
    Geometry a;
    if ((rc = rgb_rule_from_format(fmt, a.g))) return rc;
    a.lay = RgbListLayout{a.g.bps, (unsigned)a.g.ch, a.g.planar};
    a.np = (int)a.lay.planes();
    a.dw = dw;
    a.dh = dh;
    if (dw == 0 || dh == 0) return fail(SRCNN_E_SCALE, "scaled size %ux%u", dw, dh);
    if (tile_w < kDeltaTileMin || tile_w > kDeltaTileMax || tile_h < kDeltaTileMin || tile_h > kDeltaTileMax)
        return fail(SRCNN_E_ARG, "tile %ux%u: a side is %u ... %u", tile_w, tile_h, kDeltaTileMin, kDeltaTileMax);
    if (cols != (dw + tile_w - 1) / tile_w || rows != (dh + tile_h - 1) / tile_h)
        return fail(SRCNN_E_ARG, "%u x %u tiles of %ux%u do not cover %ux%u", cols, rows, tile_w, tile_h, dw, dh);
    if (!flags) return fail(SRCNN_E_ARG, "NULL flags");
    if (item_size != sizeof(srcnn_rgb_rect_item)) return fail(SRCNN_E_ARG, "item_size %u is not sizeof(srcnn_rgb_rect_item) = %zu", item_size, sizeof(srcnn_rgb_rect_item));
    if (!items && cap) return fail(SRCNN_E_ARG, "NULL items with cap = %u", cap);
    YuvPlane out[5];
    int nout = 0;
    RgbDeltaDst d;
    if ((rc = describe_destination(a, dst, dst_pitch, dst_conv, dst_conv_pitch, out, nout, d))) return rc;
    std::vector<DeltaRect> rects;
    *n = delta_coalesce(flags, cols, rows, tile_w, tile_h, dw, dh, rects);
    if (!items && cap == 0) return SRCNN_OK;         // counts only
    if (!rgb_delta_items(rects, a.lay, d, items, cap)) return fail(SRCNN_E_ARG, "%u rects do not fit %u items", *n, cap);
    return SRCNN_OK;
}

int srcnn_rgb_upscale_delta_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter, const void* const prev[4],
                                const size_t prev_pitch[4], const void* const cur[4], const size_t cur_pitch[4], unsigned tile_w,
                                unsigned tile_h, void* const dst[4], const size_t dst_pitch[4], void* dst_conv, size_t dst_conv_pitch,
                                void* stream, srcnn_delta_stats* stats)
{
    int rc, nout = 0;
    Geometry a;
    YuvPlane in_prev[4], in_cur[4], out[5];
    RgbDeltaDst d;
    if ((rc = check_geometry(fmt, w, h, multiply, filter, tile_w, tile_h, a))) return rc;
    if (stats && stats->struct_size != sizeof(srcnn_delta_stats))
        return fail(SRCNN_E_ARG, "stats->struct_size %u is not sizeof(srcnn_delta_stats) = %zu", stats->struct_size, sizeof(srcnn_delta_stats));
    if ((rc = check_sources(a, w, h, prev, prev_pitch, cur, cur_pitch, in_prev, in_cur))) return rc;
    if (!dst) return fail(SRCNN_E_ARG, "NULL plane array of the destination");
    if ((rc = describe_destination(a, dst, dst_pitch, dst_conv, dst_conv_pitch, out, nout, d))) return rc;
    if (prev && (rc = check_in_out_overlap(in_prev, a.np, out, nout))) return rc;
    if ((rc = check_in_out_overlap(in_cur, a.np, out, nout))) return rc;
    if ((rc = check_out_out_overlap(out, nout))) return rc;

    srcnn_delta_stats st{};
    st.struct_size = (unsigned)sizeof(srcnn_delta_stats);
    st.tiles = (unsigned)a.tiles();
    std::vector<DeltaRect> rects;
    {
        StreamCall sc(stream);
        if (sc.rc) return sc.rc;
        Call& c = sc.c;
        if (foreign_capture(c)) return fail(SRCNN_E_UNSUPPORTED, "srcnn_rgb_upscale_delta_dev waits for the flags: not on a stream under capture");
        if (!prev) {                                 // no previous image: the whole image, and nothing to wait for
            st.dirty_tiles = st.tiles;
            rects.push_back(DeltaRect{0, 0, a.dw, a.dh});
            st.whole_frame = 1;
        } else {
            Workspace& ws = *c.ws;
            // all scratch first: growing drains the device
            if ((rc = ws.grow(ws.delta_flags, a.tiles())) || (rc = ws.delta_stage.pin.grow(a.tiles(), *c.cx))) return rc;
            if ((rc = ensure_spans(c, w, h, filter, a))) return rc;
            TraceRange tr("srcnn rgb delta flags %ux%u tiles", a.grid.cols, a.grid.rows);
            if ((rc = queue_flags(c, a, w, h, in_prev, in_cur, ws.delta_flags.data()))) return rc;
            unsigned char* host = ws.delta_stage.pin.data();
            HIP_TRY(hipMemcpyAsync(host, ws.delta_flags.data(), a.tiles(), hipMemcpyDeviceToHost, c.s));
            if (const hipError_t e = wait_stream(c.s); e != hipSuccess) return fail(SRCNN_E_HIP, "rgb_upscale_delta: waiting for the flags: %s", hipGetErrorString(e));
            for (size_t k = 0; k < a.tiles(); ++k) st.dirty_tiles += host[k] != 0;
            delta_coalesce(host, a.grid.cols, a.grid.rows, a.grid.tile_w, a.grid.tile_h, a.dw, a.dh, rects);
        }
    }                                                // (the workspace is released: the list call takes it itself)
    st.rects = (unsigned)std::min<size_t>(rects.size(), 0xffffffffu);
    st.cell_samples = delta_cell_samples(rects);
    if (delta_whole_frame(rects.size(), st.dirty_tiles, st.tiles, st.cell_samples, a.dw, a.dh, settings().delta_whole_permille)) {
        st.whole_frame = 1;
        rects.assign(1, DeltaRect{0, 0, a.dw, a.dh});
    }
    if (stats) *stats = st;
    if (rects.empty()) return SRCNN_OK;
    std::vector<srcnn_rgb_rect_item> items(rects.size());
    rgb_delta_items(rects, a.lay, d, items.data(), items.size());
    return srcnn_rgb_upscale_rect_list_dev(fmt, w, h, multiply, filter, cur, cur_pitch, items.data(), (unsigned)items.size(),
                                           (unsigned)sizeof(srcnn_rgb_rect_item), stream);
}

}  // extern "C"
