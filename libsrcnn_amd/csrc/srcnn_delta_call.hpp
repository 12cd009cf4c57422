// srcnn_delta_call.hpp -- the host skeleton under the two delta calls (Y plane: srcnn_delta_call.cpp, RGB(A):
// srcnn_rgb_delta_call.cpp).  What a delta call is whatever its surface: the span tables of a stream's workspace and when they are
// uploaded, the flags call, and the whole operation -- scratch, tables, the flags kernel, the one wait, the plan of
// srcnn_delta.hpp, the repaint through the surface's rect list call.  The argument checks stay with each call: their order is
// public.  Internal.
//
// A Surface, which a call file builds once its arguments have passed, has
//   w, h, dw, dh, filter, grid   the geometry and the DeltaGrid
//   kOwner                       whose span tables it builds (DeltaSpanOwner, srcnn_host.hpp)
//   kTrace, kName, kEntry        the trace label, and the whole operation's name in its two messages
//   has_prev()                   false: no previous frame
//   spans(c, xs, ys)             its contribution tables (get_table) through its span builder
//   queue_flags(c, d_flags)      the launch of its flags kernel over ws.delta_spans, with its name in the SRCNN_E_HIP message
//   repaint(rects, stream)       the rects as items of its public rect list call, and that call
#pragma once
#include <cstring>
#include <vector>

#include "srcnn_delta.hpp"
#include "srcnn_rect_list_call.hpp"

namespace srcnn {

inline int check_delta_stats(const srcnn_delta_stats* stats)
{
    if (stats && stats->struct_size != sizeof(srcnn_delta_stats))
        return fail(SRCNN_E_ARG, "stats->struct_size %u is not sizeof(srcnn_delta_stats) = %zu", stats->struct_size, sizeof(srcnn_delta_stats));
    return SRCNN_OK;
}

// The span tables of the surface's geometry in the workspace, uploaded when the geometry or the owner changes.  The copy is
// ordered on the call's stream, behind any kernel that still reads the old tables, and has landed when it returns.
template <class Surface>
int ensure_delta_spans(Call& c, const Surface& sf)
{
    Workspace& ws = *c.ws;
    DeltaStage& st = ws.delta_stage;
    const DeltaGrid& g = sf.grid;
    const unsigned key[7] = {sf.w, sf.h, sf.dw, sf.dh, (unsigned)sf.filter, g.tile_w, g.tile_h};
    static_assert(sizeof key == sizeof st.key, "the geometry key");
    const size_t words = delta_span_words(g.cols, g.rows);
    if (st.valid && st.owner == Surface::kOwner && !memcmp(st.key, key, sizeof key) && ws.delta_spans.size() >= words) return SRCNN_OK;
    if (foreign_capture(c))
        return fail(SRCNN_E_UNSUPPORTED, "the span tables of %ux%u -> %ux%u are not on the device yet, and the stream is being captured: run the call once outside the capture", sf.w, sf.h, sf.dw, sf.dh);
    int rc;
    std::vector<DeltaSpan> xs, ys;
    if ((rc = sf.spans(c, xs, ys))) return rc;
    if (!delta_spans_monotone(xs, sf.w) || !delta_spans_monotone(ys, sf.h))
        return fail(SRCNN_E_UNSUPPORTED, "the tile spans of %ux%u -> %ux%u (filter %d) are not monotone", sf.w, sf.h, sf.dw, sf.dh, sf.filter);
    std::vector<unsigned> image(words);
    delta_span_image(xs, ys, image.data());
    st.valid = false;
    if ((rc = ws.grow(ws.delta_spans, words))) return rc;
    if ((rc = copy_h2d_any(*c.cx, ws.delta_spans.data(), image.data(), sizeof(unsigned) * words, c.s))) return rc;
    memcpy(st.key, key, sizeof key);
    st.owner = Surface::kOwner;
    st.valid = true;
    return SRCNN_OK;
}

// the *_flags_dev entry point of a surface, after its checks: asynchronous on `stream`
template <class Surface>
int delta_flags_call(const Surface& sf, unsigned char* d_flags, void* stream)
{
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    Call& c = sc.c;
    if (!sf.has_prev()) {                            // no previous frame: everything is dirty
        HIP_TRY(hipMemsetAsync(d_flags, 1, (size_t)sf.grid.cols * sf.grid.rows, c.s));
        return SRCNN_OK;
    }
    if (const int rc = ensure_delta_spans(c, sf)) return rc;
    return sf.queue_flags(c, d_flags);
}

// the whole operation of a surface, after its checks; *stats (may be NULL) is written before anything is repainted
template <class Surface>
int delta_call(const Surface& sf, void* stream, srcnn_delta_stats* stats)
{
    srcnn_delta_stats st;
    std::vector<DeltaRect> rects;
    {
        int rc;
        StreamCall sc(stream);
        if (sc.rc) return sc.rc;
        Call& c = sc.c;
        if (foreign_capture(c)) return fail(SRCNN_E_UNSUPPORTED, "%s waits for the flags: not on a stream under capture", Surface::kEntry);
        const unsigned char* host = nullptr;         // no previous frame: the whole frame, and nothing to wait for
        if (sf.has_prev()) {
            Workspace& ws = *c.ws;
            const size_t tiles = (size_t)sf.grid.cols * sf.grid.rows;
            // all scratch first: growing drains the device
            if ((rc = ws.grow(ws.delta_flags, tiles)) || (rc = ws.delta_stage.pin.grow(tiles, *c.cx))) return rc;
            if ((rc = ensure_delta_spans(c, sf))) return rc;
            TraceRange tr("srcnn %s flags %ux%u tiles", Surface::kTrace, sf.grid.cols, sf.grid.rows);
            if ((rc = sf.queue_flags(c, ws.delta_flags.data()))) return rc;
            HIP_TRY(hipMemcpyAsync(ws.delta_stage.pin.data(), ws.delta_flags.data(), tiles, hipMemcpyDeviceToHost, c.s));
            // the one wait of the call
            if (const hipError_t e = wait_stream(c.s); e != hipSuccess) return fail(SRCNN_E_HIP, "%s: waiting for the flags: %s", Surface::kName, hipGetErrorString(e));
            host = ws.delta_stage.pin.data();
        }
        delta_plan(host, sf.grid, sf.dw, sf.dh, settings().delta_whole_permille, st, rects);
    }                                                // (the workspace is released: the list call takes it itself)
    if (stats) *stats = st;
    if (rects.empty()) return SRCNN_OK;
    return sf.repaint(rects, stream);
}

}  // namespace srcnn
