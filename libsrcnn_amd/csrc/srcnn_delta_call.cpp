// srcnn_delta_call.cpp -- the delta call (include/srcnn_amd_delta.h): its argument checks, the span tables of a stream's
// workspace, the launch of k_delta_flags (srcnn_delta.hip) and, for the whole operation, the one wait for the flags, the
// coalescer and the whole-frame rule of srcnn_delta.hpp, and the rect list call that repaints.  Nothing of the list call, the
// rect call or their kernels is changed: the rects go through the public srcnn_y_path_rect_list_f32_dev.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/srcnn_amd_delta.h"
#include "srcnn_delta.h"
#include "srcnn_delta.hpp"
#include "srcnn_frame_args.hpp"
#include "srcnn_rect_list_call.hpp"

using namespace srcnn;

namespace {

// the source planes and the grid: what both device entry points refuse before any device lookup
struct DeltaArgs {
    DeltaGrid g;
    YuvPlane prev, cur;
    size_t tiles() const { return (size_t)g.cols * g.rows; }
};

int check_delta_sources(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h, unsigned dw,
                        unsigned dh, int filter, unsigned tile_w, unsigned tile_h, DeltaArgs& a)
{
    int rc;
    if (!d_cur) return fail(SRCNN_E_ARG, "NULL d_cur");
    if ((rc = delta_grid(w, h, dw, dh, filter, tile_w, tile_h, a.g))) return rc;
    if (d_prev && (rc = describe_plane(a.prev, d_prev, prev_pitch, sizeof(float) * (size_t)w, h, 4, "previous", 0))) return rc;
    return describe_plane(a.cur, d_cur, cur_pitch, sizeof(float) * (size_t)w, h, 4, "current", 0);
}

// The span tables of this geometry in the workspace, uploaded when the geometry changes.  The copy is ordered on the call's
// stream, behind any kernel that still reads the old tables, and has landed when it returns.
int ensure_spans(Call& c, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const DeltaGrid& g)
{
    Workspace& ws = *c.ws;
    DeltaStage& st = ws.delta_stage;
    const unsigned key[8] = {w, h, dw, dh, (unsigned)filter, g.tile_w, g.tile_h, 0};
    const size_t words = delta_span_words(g.cols, g.rows);
    if (st.valid && !memcmp(st.key, key, sizeof key) && ws.delta_spans.size() >= words) return SRCNN_OK;
    if (foreign_capture(c))
        return fail(SRCNN_E_UNSUPPORTED, "the span tables of %ux%u -> %ux%u are not on the device yet, and the stream is being captured: run the call once outside the capture", w, h, dw, dh);
    int rc;
    std::vector<DeltaSpan> xs, ys;
    TableRef th, tv;
    if (dw != w && (rc = get_table(c, filter, dw, w, th))) return rc;
    if (dh != h && (rc = get_table(c, filter, dh, h, tv))) return rc;
    delta_axis_spans(th ? th->h_first.data() : nullptr, th ? th->h_taps.data() : nullptr, dw, w, g.tile_w, xs);
    delta_axis_spans(tv ? tv->h_first.data() : nullptr, tv ? tv->h_taps.data() : nullptr, dh, h, g.tile_h, ys);
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

int queue_flags(Call& c, const float* d_prev, const float* d_cur, const DeltaArgs& a, unsigned w, unsigned h, unsigned char* d_flags)
{
    launch_delta_flags(d_prev, a.prev.pitch, d_cur, a.cur.pitch, w, h, c.ws->delta_spans.data(), a.g.cols, a.g.rows, d_flags, c.s);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail(SRCNN_E_HIP, "y_path_delta_flags: %s", hipGetErrorString(e));
    return SRCNN_OK;
}

}  // namespace

extern "C" {

int srcnn_delta_abi_version(void) { return SRCNN_AMD_DELTA_VERSION; }

int srcnn_y_path_delta_grid(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h, unsigned* cols,
                            unsigned* rows)
{
    if (!cols || !rows) return fail(SRCNN_E_ARG, "NULL cols or rows");
    DeltaGrid g;
    if (const int rc = delta_grid(w, h, dw, dh, filter, tile_w, tile_h, g)) return rc;
    *cols = g.cols;
    *rows = g.rows;
    return SRCNN_OK;
}

int srcnn_y_path_delta_flags_dev(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h,
                                 unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h, unsigned char* d_flags, void* stream)
{
    int rc;
    DeltaArgs a;
    if (!d_flags) return fail(SRCNN_E_ARG, "NULL d_flags");
    if ((rc = check_delta_sources(d_prev, prev_pitch, d_cur, cur_pitch, w, h, dw, dh, filter, tile_w, tile_h, a))) return rc;
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    Call& c = sc.c;
    if (!d_prev) {                                   // no previous frame: everything is dirty
        HIP_TRY(hipMemsetAsync(d_flags, 1, a.tiles(), c.s));
        return SRCNN_OK;
    }
    if ((rc = ensure_spans(c, w, h, dw, dh, filter, a.g))) return rc;
    return queue_flags(c, d_prev, d_cur, a, w, h, d_flags);
}

int srcnn_y_path_delta_rects(const unsigned char* flags, unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h, unsigned dw,
                             unsigned dh, float* d_out, size_t out_pitch, srcnn_rect_item* items, unsigned cap, unsigned* n)
{
    if (!n) return fail(SRCNN_E_ARG, "NULL n");
    *n = 0;
    if (dw == 0 || dh == 0) return fail(SRCNN_E_SCALE, "scaled size %ux%u", dw, dh);
    if (tile_w < kDeltaTileMin || tile_w > kDeltaTileMax || tile_h < kDeltaTileMin || tile_h > kDeltaTileMax)
        return fail(SRCNN_E_ARG, "tile %ux%u: a side is %u ... %u", tile_w, tile_h, kDeltaTileMin, kDeltaTileMax);
    if (cols != (dw + tile_w - 1) / tile_w || rows != (dh + tile_h - 1) / tile_h)
        return fail(SRCNN_E_ARG, "%u x %u tiles of %ux%u do not cover %ux%u", cols, rows, tile_w, tile_h, dw, dh);
    if (!flags) return fail(SRCNN_E_ARG, "NULL flags");
    if (!items && cap) return fail(SRCNN_E_ARG, "NULL items with cap = %u", cap);
    YuvPlane out;
    if (const int rc = describe_plane(out, d_out, out_pitch, sizeof(float) * (size_t)dw, dh, 4, "output", 0)) return rc;
    std::vector<DeltaRect> rects;
    *n = delta_coalesce(flags, cols, rows, tile_w, tile_h, dw, dh, rects);
    if (!items && cap == 0) return SRCNN_OK;         // counts only
    if (!delta_items(rects, d_out, out.pitch, items, cap)) return fail(SRCNN_E_ARG, "%u rects do not fit %u items", *n, cap);
    return SRCNN_OK;
}

int srcnn_y_path_delta_f32_dev(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h,
                               unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h, float* d_out, size_t out_pitch,
                               void* stream, srcnn_delta_stats* stats)
{
    int rc;
    DeltaArgs a;
    YuvPlane out;
    if (!d_out) return fail(SRCNN_E_ARG, "NULL d_out");
    if (stats && stats->struct_size != sizeof(srcnn_delta_stats))
        return fail(SRCNN_E_ARG, "stats->struct_size %u is not sizeof(srcnn_delta_stats) = %zu", stats->struct_size, sizeof(srcnn_delta_stats));
    if ((rc = check_delta_sources(d_prev, prev_pitch, d_cur, cur_pitch, w, h, dw, dh, filter, tile_w, tile_h, a))) return rc;
    if ((rc = describe_plane(out, d_out, out_pitch, sizeof(float) * (size_t)dw, dh, 4, "output", 0))) return rc;
    if (d_prev && overlaps(a.prev, out)) return fail(SRCNN_E_ARG, "d_out overlaps d_prev");
    if (overlaps(a.cur, out)) return fail(SRCNN_E_ARG, "d_out overlaps d_cur");

    srcnn_delta_stats st{};
    st.struct_size = (unsigned)sizeof(srcnn_delta_stats);
    st.tiles = (unsigned)a.tiles();
    std::vector<DeltaRect> rects;
    {
        StreamCall sc(stream);
        if (sc.rc) return sc.rc;
        Call& c = sc.c;
        if (foreign_capture(c)) return fail(SRCNN_E_UNSUPPORTED, "srcnn_y_path_delta_f32_dev waits for the flags: not on a stream under capture");
        if (!d_prev) {                               // no previous frame: the whole frame, and nothing to wait for
            st.dirty_tiles = st.tiles;
            rects.push_back(DeltaRect{0, 0, dw, dh});
            st.whole_frame = 1;
        } else {
            Workspace& ws = *c.ws;
            // all scratch first: growing drains the device
            if ((rc = ws.grow(ws.delta_flags, a.tiles())) || (rc = ws.delta_stage.pin.grow(a.tiles(), *c.cx))) return rc;
            if ((rc = ensure_spans(c, w, h, dw, dh, filter, a.g))) return rc;
            TraceRange tr("srcnn delta flags %ux%u tiles", a.g.cols, a.g.rows);
            if ((rc = queue_flags(c, d_prev, d_cur, a, w, h, ws.delta_flags.data()))) return rc;
            unsigned char* host = ws.delta_stage.pin.data();
            HIP_TRY(hipMemcpyAsync(host, ws.delta_flags.data(), a.tiles(), hipMemcpyDeviceToHost, c.s));
            if (const hipError_t e = wait_stream(c.s); e != hipSuccess) return fail(SRCNN_E_HIP, "y_path_delta: waiting for the flags: %s", hipGetErrorString(e));
            for (size_t k = 0; k < a.tiles(); ++k) st.dirty_tiles += host[k] != 0;
            delta_coalesce(host, a.g.cols, a.g.rows, a.g.tile_w, a.g.tile_h, dw, dh, rects);
        }
    }                                                // (the workspace is released: the list call takes it itself)
    st.rects = (unsigned)std::min<size_t>(rects.size(), 0xffffffffu);
    st.cell_samples = delta_cell_samples(rects);
    if (delta_whole_frame(rects.size(), st.dirty_tiles, st.tiles, st.cell_samples, dw, dh, settings().delta_whole_permille)) {
        st.whole_frame = 1;
        rects.assign(1, DeltaRect{0, 0, dw, dh});
    }
    if (stats) *stats = st;
    if (rects.empty()) return SRCNN_OK;
    std::vector<srcnn_rect_item> items(rects.size());
    delta_items(rects, d_out, out.pitch, items.data(), items.size());
    return srcnn_y_path_rect_list_f32_dev(d_cur, cur_pitch, w, h, dw, dh, filter, items.data(), (unsigned)items.size(), (unsigned)sizeof(srcnn_rect_item), stream);
}

}  // extern "C"
