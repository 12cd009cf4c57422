// srcnn_yuv_packed_rect_list_call.cpp -- the packed YUV rect LIST call (include/srcnn_amd_yuv_packed_rect_list.h): argument
// checks, routing and packing (srcnn_rect_atlas.hpp with the chroma condition of srcnn_yuv_packed_rect_atlas.hpp), the upload of
// the two descriptor tables and the six launches of an atlas (srcnn_yuv_packed_rect_list.hip around the list's replicate and the
// unchanged layer kernels).  Single items go through yuv_packed_rect of srcnn_frames.cpp, exactly as the single call runs it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/srcnn_amd_yuv_packed_rect_list.h"
#include "resample_table.hpp"
#include "srcnn_frame_args.hpp"
#include "srcnn_host.hpp"
#include "srcnn_rect_list.h"
#include "srcnn_rect_source.hpp"
#include "srcnn_yuv.h"
#include "srcnn_yuv_packed_rect_atlas.hpp"

using namespace srcnn;

namespace {

static_assert(sizeof(srcnn_yuv_packed_rect_item) == 32 || sizeof(void*) != 8, "the header states 32 B per item on LP64");
static_assert(sizeof(ListCellDesc) == 80 && sizeof(YuvPackedListDstDesc) == 64, "the header states 80 + 64 B per batched item");

// the failure of item k, with the index in front of what the single call would have said
int fail_item(int rc, unsigned k)
{
    const std::string why = last_error();
    return fail(rc, "item %u: %s", k, why.c_str());
}

// What both entry points refuse about the list itself.  SRCNN_OK with n == 0: nothing to do.
int check_list(const srcnn_yuv_packed_rect_item* items, unsigned n, unsigned item_size)
{
    if (item_size != sizeof(srcnn_yuv_packed_rect_item))
        return fail(SRCNN_E_ARG, "item_size %u is not sizeof(srcnn_yuv_packed_rect_item) = %zu", item_size, sizeof(srcnn_yuv_packed_rect_item));
    if (n == 0) return SRCNN_OK;
    if (!items) return fail(SRCNN_E_ARG, "NULL items with n = %u", n);
    if (n > kRectListMax) return fail(SRCNN_E_UNSUPPORTED, "%u items: a list holds at most %u", n, kRectListMax);
    return SRCNN_OK;
}

YuvPackedRouteInputs route_inputs(int kind, unsigned w, unsigned h, unsigned dw, unsigned dh, int mode, bool foreign_capture)
{
    YuvPackedRouteInputs in;
    in.kind = kind;
    in.y.w = w; in.y.h = h; in.y.dw = dw; in.y.dh = dh;
    in.y.strict = mode == SRCNN_MODE_STRICT;
    in.y.unfused = foreign_capture || settings().yuv_packed_rect_list_unfused;
    in.y.cap_bytes = G.ws_budget.load();
    in.y.single_samples = settings().rect_list_single_samples > 0 ? (unsigned long long)settings().rect_list_single_samples : 0;
    return in;
}
bool may_batch(const YuvPackedRouteInputs& in) { return in.y.strict && !in.y.unfused && in.y.dw > in.y.w && in.y.dh > in.y.h && in.chroma_grows(); }

unsigned long long largest_atlas(const RectListRoute& route)
{
    unsigned long long largest = 0;
    for (const AtlasPass& p : route.passes) largest = std::max(largest, (unsigned long long)p.W * p.H);
    return largest;
}

struct Tables { TableRef th, tv, cth, ctv; };       // Y: (dw <- w), (dh <- h); chroma: (dcw <- cw), (dh <- h) with chroma_filter

struct Source {
    const YuvPackedGeom& g;
    const YuvPlane& in;                              // the WHOLE frame
    unsigned w, h;
};

// One atlas: the six launches.  d / dd: the device copies of the pass's cell and destination tables, hd / hdd: the host copies.
int list_pass(Call& c, const Source& s, const Tables& t, const AtlasPass& pass, const ListCellDesc* d, const YuvPackedListDstDesc* dd,
              const ListCellDesc* hd, const YuvPackedListDstDesc* hdd)
{
    Workspace& ws = *c.ws;
    const ListCellDesc& end = hd[pass.count];
    const unsigned W = pass.W, H = pass.H;
    const size_t plane = (size_t)W * H;
    TraceRange tr("srcnn yuv packed rect list atlas %ux%u, %u cells", W, H, pass.count);
    {
        StageTimer st(SRCNN_STAGE_RESAMPLE, c);
        launch_yuvp_list_resample(s.g.rule, s.in.lo, s.in.pitch, s.w, s.h, t.th->view(), t.tv->view(), d, pass.count, end, ws.up.data(), W, c.s);
        launch_list_replicate(d, pass.count, end, ws.up.data(), W, 0, 1, kCellMargin, c.s);
    }
    {
        StageTimer st(SRCNN_STAGE_CONV12, c);
        run_conv12(c, ws.up.data(), (int)W, (int)H, 0, (int)H, ws.c2.data(), plane, 0, (int)H);
    }
    {
        StageTimer st(SRCNN_STAGE_CONV3, c);
        // (the ring of 2 of layer-2 activations around a rect that lies outside the plane: as in the Y list)
        launch_list_replicate(d, pass.count, end, ws.c2.data(), W, plane, C2N, 2, c.s);
        launch_layer3(ws.c2.data(), plane, (int)W, (int)H, 0, (int)H, ws.win.data(), 0, (int)H, c.relax(), c.s);
    }
    launch_yuvp_list_merge(s.g.rule, s.in.lo, s.in.pitch, s.w, s.h, t.cth->view(), t.ctv->view(), d, dd, pass.count, hdd[pass.count], ws.win.data(), W,
                           c.s);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
        ws.queue_dirty = true;
        return fail(SRCNN_E_HIP, "yuv_packed_upscale_rect_list: %s", hipGetErrorString(e));
    }
    return SRCNN_OK;
}

// The batched route: the cell tables of every pass, then the destination tables of every pass, go to the device in ONE copy, in
// stream order, from a page-locked slot that belongs to this call until its event has passed (ListStaging, srcnn_host.hpp).
int list_batched(Call& c, const Source& s, unsigned dw, unsigned dh, const Tables& t, const TileAxis& cth, const RectListRoute& route,
                 const ListRect* rects, const YuvPackedListDst* dsts)
{
    Workspace& ws = *c.ws;
    int rc;
    const size_t entries = route.cells.size() + route.passes.size();
    const size_t cell_bytes = entries * sizeof(ListCellDesc), bytes = (size_t)yuv_packed_list_desc_bytes(route);
    // all scratch first: growing drains the device, which nothing queued below may see half way
    const size_t largest = (size_t)largest_atlas(route);
    if ((rc = ws.grow(ws.up, largest)) || (rc = ws.grow(ws.win, largest)) || (rc = ws.grow(ws.c2, (size_t)C2N * largest)) || (rc = ws.grow(ws.list, bytes))) return rc;
    ListStaging::Slot& slot = ws.list_stage.slot[ws.list_stage.next];
    ws.list_stage.next = (ws.list_stage.next + 1) % ListStaging::kSlots;
    if (slot.pending) {
        if (wait_event(slot.ev.get()) != hipSuccess) return fail(SRCNN_E_HIP, "an earlier descriptor upload of this stream failed");
        slot.pending = false;
    }
    if ((rc = slot.pin.grow(bytes, *c.cx))) return rc;
    if (!slot.ev) HIP_TRY(hipEventCreateWithFlags(slot.ev.put(), hipEventDisableTiming));
    ListCellDesc* host = reinterpret_cast<ListCellDesc*>(slot.pin.data());
    YuvPackedListDstDesc* host_dst = reinterpret_cast<YuvPackedListDstDesc*>(slot.pin.data() + cell_bytes);      // (80 is a multiple of 8)
    std::vector<ListCellDesc> one;
    std::vector<YuvPackedListDstDesc> one_dst;
    std::vector<size_t> at;                        // first entry of each pass, the same in both tables
    size_t pos = 0;
    for (const AtlasPass& p : route.passes) {
        if (!build_cell_descs(route, p, rects, nullptr, dw, dh, one) || one.back().rs_tile0 > 0x7fffffffu || one.back().rep_tile0 > 0x7fffffffu ||
            !build_yuv_packed_dst_descs(route, p, rects, dsts, s.g.rule.kind, s.w, dw, cth, one_dst) || one_dst.back().ch_tile0 > 0x7fffffffu)
            return fail(SRCNN_E_UNSUPPORTED, "an atlas of %u cells has more tiles than one launch takes", p.count);
        memcpy(host + pos, one.data(), one.size() * sizeof(ListCellDesc));
        memcpy(host_dst + pos, one_dst.data(), one_dst.size() * sizeof(YuvPackedListDstDesc));
        at.push_back(pos);
        pos += one.size();
    }
    unsigned char* dev = ws.list.data();
    HIP_TRY(hipMemcpyAsync(dev, slot.pin.data(), bytes, hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipEventRecord(slot.ev.get(), c.s));
    slot.pending = true;
    const ListCellDesc* dev_cells = reinterpret_cast<const ListCellDesc*>(dev);
    const YuvPackedListDstDesc* dev_dst = reinterpret_cast<const YuvPackedListDstDesc*>(dev + cell_bytes);
    for (size_t k = 0; k < route.passes.size(); ++k)
        if ((rc = list_pass(c, s, t, route.passes[k], dev_cells + at[k], dev_dst + at[k], host + at[k], host_dst + at[k]))) return rc;
    return SRCNN_OK;
}

}  // namespace

extern "C" {

int srcnn_yuv_packed_rect_list_abi_version(void) { return SRCNN_AMD_YUV_PACKED_RECT_LIST_VERSION; }

int srcnn_yuv_packed_upscale_rect_list_plan(int format, unsigned w, unsigned h, float multiply, int filter, const srcnn_yuv_packed_rect_item* items,
                                            unsigned n, unsigned item_size, srcnn_rect_list_plan* plan)
{
    int rc;
    if (!plan) return fail(SRCNN_E_ARG, "NULL plan");
    if (plan->struct_size != sizeof(srcnn_rect_list_plan))
        return fail(SRCNN_E_ARG, "plan->struct_size %u is not sizeof(srcnn_rect_list_plan) = %zu", plan->struct_size, sizeof(srcnn_rect_list_plan));
    if ((rc = check_list(items, n, item_size))) return rc;
    srcnn_rect_list_plan out{};
    out.struct_size = (unsigned)sizeof(srcnn_rect_list_plan);
    if (n == 0) { *plan = out; return SRCNN_OK; }
    YuvPackedGeom g;
    unsigned dw = 0, dh = 0;
    if ((rc = yuv_packed_geom(format, g))) return rc;
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    std::vector<ListRect> rects(n);
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_yuv_packed_rect_item& it = items[k];
        if ((rc = check_yuv_packed_rect_place(g, dw, dh, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
    }
    YuvPackedRouteInputs in = route_inputs(g.rule.kind, w, h, dw, dh, G.mode.load(), false);
    AxisTable th, tv, cth, ctv;
    if (may_batch(in)) {
        const int cfilter = chroma_filter(filter);
        th = build_axis_table(filter, dw, w);
        tv = build_axis_table(filter, dh, h);
        cth = build_axis_table(cfilter, g.ccols(dw), g.ccols(w));
        ctv = build_axis_table(cfilter, dh, h);
        in.y.th = TileAxis{th.first.data(), th.taps.data(), th.max_taps};
        in.y.tv = TileAxis{tv.first.data(), tv.taps.data(), tv.max_taps};
        in.cth = TileAxis{cth.first.data(), cth.taps.data(), cth.max_taps};
        in.ctv = TileAxis{ctv.first.data(), ctv.taps.data(), ctv.max_taps};
    }
    const RectListRoute route = route_yuv_packed_rect_list(rects.data(), n, in);
    out.batched_items = (unsigned)route.cells.size();
    out.single_items = (unsigned)route.single.size();
    out.atlases = (unsigned)route.passes.size();
    out.cell_samples = route.cell_samples;
    out.atlas_samples = route.atlas_samples;
    out.scratch_bytes = largest_atlas(route) * (kAtlasSampleBytes + 8) + yuv_packed_list_desc_bytes(route);
    *plan = out;
    return SRCNN_OK;
}

int srcnn_yuv_packed_upscale_rect_list_dev(int format, unsigned w, unsigned h, float multiply, int filter, const void* src, size_t src_pitch,
                                           const srcnn_yuv_packed_rect_item* items, unsigned n, unsigned item_size, void* stream)
{
    int rc;
    if ((rc = check_list(items, n, item_size))) return rc;
    if (n == 0) return SRCNN_OK;
    // the frame, in the order of srcnn_yuv_packed_upscale_rect_dev
    YuvPackedGeom g;
    unsigned dw = 0, dh = 0;
    if ((rc = yuv_packed_geom(format, g))) return rc;
    if (!src) return fail(SRCNN_E_ARG, "NULL frame");
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    YuvPlane in;
    if ((rc = describe_yuv_packed_source(g, w, h, src, src_pitch, in))) return rc;
    // every item with the single call's per-rect rules, in its order; nothing has been queued yet
    std::vector<ListRect> rects(n);
    std::vector<YuvPackedListDst> dsts(n);
    std::vector<YuvPlane> outs(n);
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_yuv_packed_rect_item& it = items[k];
        if (!it.dst) return fail(SRCNN_E_ARG, "item %u: NULL frame", k);
        if ((rc = check_yuv_packed_rect_place(g, dw, dh, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        if ((rc = check_yuv_packed_rect_dst(g, dw, it.x0, it.rw, it.rh, it.dst, it.dst_pitch, in, outs[k]))) return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
        dsts[k] = YuvPackedListDst{it.dst, outs[k].pitch};
    }
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    Call& c = sc.c;
    // a capture that is not the library's own, as run_conv12 detects it: the descriptor upload and the tile queue stay out of it
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool foreign_capture = c.s && c.ws && !c.ws->frozen && hipStreamIsCapturing(c.s, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive;
    YuvPackedRouteInputs ri = route_inputs(g.rule.kind, w, h, dw, dh, c.mode, foreign_capture);
    Tables t;
    if (may_batch(ri)) {
        const int cfilter = chroma_filter(filter);
        if ((rc = get_table(c, filter, dw, w, t.th)) || (rc = get_table(c, filter, dh, h, t.tv)) ||
            (rc = get_table(c, cfilter, g.ccols(dw), g.ccols(w), t.cth)) || (rc = get_table(c, cfilter, dh, h, t.ctv)))
            return rc;
        ri.y.th = TileAxis{t.th->h_first.data(), t.th->h_taps.data(), t.th->max_taps};
        ri.y.tv = TileAxis{t.tv->h_first.data(), t.tv->h_taps.data(), t.tv->max_taps};
        ri.cth = TileAxis{t.cth->h_first.data(), t.cth->h_taps.data(), t.cth->max_taps};
        ri.ctv = TileAxis{t.ctv->h_first.data(), t.ctv->h_taps.data(), t.ctv->max_taps};
    }
    const RectListRoute route = route_yuv_packed_rect_list(rects.data(), n, ri);
    const Source s{g, in, w, h};
    if (!route.cells.empty() && (rc = list_batched(c, s, dw, dh, t, ri.cth, route, rects.data(), dsts.data()))) return rc;
    for (unsigned k : route.single) {
        const ListRect& r = rects[k];
        if ((rc = yuv_packed_rect(c, g, w, h, dw, dh, filter, in, outs[k], r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh))) return rc;
    }
    return SRCNN_OK;
}

}  // extern "C"
