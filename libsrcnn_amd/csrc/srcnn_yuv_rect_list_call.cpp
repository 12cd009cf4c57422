// srcnn_yuv_rect_list_call.cpp -- the planar / semi-planar YUV rect LIST call (include/srcnn_amd_yuv_rect_list.h): argument
// checks, routing and packing (srcnn_rect_atlas.hpp with the chroma condition of srcnn_yuv_rect_atlas.hpp), the upload of the
// two descriptor tables and the seven launches of an atlas (srcnn_yuv_rect_list.hip around the list's replicate and the
// unchanged layer kernels).  Single items go through yuv_rect of srcnn_frames.cpp, exactly as the single call runs it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/srcnn_amd_yuv_rect_list.h"
#include "resample_table.hpp"
#include "srcnn_frame_args.hpp"
#include "srcnn_host.hpp"
#include "srcnn_rect_list.h"
#include "srcnn_rect_source.hpp"
#include "srcnn_yuv.h"
#include "srcnn_yuv_rect_atlas.hpp"

using namespace srcnn;

namespace {

static_assert(sizeof(srcnn_yuv_rect_item) == 64 || sizeof(void*) != 8, "the header states 64 B per item on LP64");
static_assert(sizeof(ListCellDesc) == 80 && sizeof(YuvListDstDesc) == 80, "the header states 80 + 80 B per batched item");

// the failure of item k, with the index in front of what the single call would have said
int fail_item(int rc, unsigned k)
{
    const std::string why = last_error();
    return fail(rc, "item %u: %s", k, why.c_str());
}

// What both entry points refuse about the list itself.  SRCNN_OK with n == 0: nothing to do.
int check_list(const srcnn_yuv_rect_item* items, unsigned n, unsigned item_size)
{
    if (item_size != sizeof(srcnn_yuv_rect_item))
        return fail(SRCNN_E_ARG, "item_size %u is not sizeof(srcnn_yuv_rect_item) = %zu", item_size, sizeof(srcnn_yuv_rect_item));
    if (n == 0) return SRCNN_OK;
    if (!items) return fail(SRCNN_E_ARG, "NULL items with n = %u", n);
    if (n > kRectListMax) return fail(SRCNN_E_UNSUPPORTED, "%u items: a list holds at most %u", n, kRectListMax);
    return SRCNN_OK;
}

YuvRouteInputs route_inputs(const YuvGeom& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int mode, bool foreign_capture)
{
    YuvRouteInputs in;
    in.g = g;
    in.y.w = w; in.y.h = h; in.y.dw = dw; in.y.dh = dh;
    in.y.strict = mode == SRCNN_MODE_STRICT;
    in.y.unfused = foreign_capture || settings().yuv_rect_list_unfused;
    in.y.cap_bytes = G.ws_budget.load();
    in.y.single_samples = settings().rect_list_single_samples > 0 ? (unsigned long long)settings().rect_list_single_samples : 0;
    return in;
}
bool may_batch(const YuvRouteInputs& in) { return in.y.strict && !in.y.unfused && in.y.dw > in.y.w && in.y.dh > in.y.h && in.chroma_grows(); }

unsigned long long largest_atlas(const RectListRoute& route)
{
    unsigned long long largest = 0;
    for (const AtlasPass& p : route.passes) largest = std::max(largest, (unsigned long long)p.W * p.H);
    return largest;
}

struct Tables { TableRef th, tv, cth, ctv; };       // Y: (dw <- w), (dh <- h); chroma: (dcw <- cw), (dch <- ch) with chroma_filter

struct Source {
    const YuvGeom& g;
    const YuvPlane* in;                              // the WHOLE frame's planes
    unsigned w, h;
};

// One atlas: the seven launches.  d / dd: the device copies of the pass's cell and destination tables, hd / hdd: the host copies.
int list_pass(Call& c, const Source& s, const Tables& t, const AtlasPass& pass, const ListCellDesc* d, const YuvListDstDesc* dd, const ListCellDesc* hd,
              const YuvListDstDesc* hdd)
{
    Workspace& ws = *c.ws;
    const ListCellDesc& end = hd[pass.count];
    const unsigned W = pass.W, H = pass.H;
    const size_t plane = (size_t)W * H;
    const Yuv16Rule* rule = s.g.bps == 2 ? &s.g.rule : nullptr;
    TraceRange tr("srcnn yuv rect list atlas %ux%u, %u cells", W, H, pass.count);
    {
        StageTimer st(SRCNN_STAGE_RESAMPLE, c);
        launch_yuv_list_resample(s.in[0].lo, s.in[0].pitch, s.w, s.h, rule, t.th->view(), t.tv->view(), d, pass.count, end, ws.up.data(), W, c.s);
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
    launch_yuv_list_luma(rule, d, dd, pass.count, end, ws.win.data(), W, c.s);
    const unsigned char* csrc[2] = {s.in[1].lo, s.in[2].lo};
    const size_t cspitch[2] = {s.in[1].pitch, s.in[2].pitch};
    launch_yuv_list_chroma(csrc, cspitch, s.g.ccols(s.w), s.g.crows(s.h), s.g.semi, rule, t.cth->view(), t.ctv->view(), dd, pass.count, hdd[pass.count], c.s);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
        ws.queue_dirty = true;
        return fail(SRCNN_E_HIP, "yuv_upscale_rect_list: %s", hipGetErrorString(e));
    }
    return SRCNN_OK;
}

// The batched route: the cell tables of every pass, then the destination tables of every pass, go to the device in ONE copy, in
// stream order, from a page-locked slot that belongs to this call until its event has passed (ListStaging, srcnn_host.hpp).
int list_batched(Call& c, const Source& s, unsigned dw, unsigned dh, const Tables& t, const RectListRoute& route, const ListRect* rects,
                 const YuvListDst* dsts)
{
    Workspace& ws = *c.ws;
    int rc;
    const size_t entries = route.cells.size() + route.passes.size();
    const size_t cell_bytes = entries * sizeof(ListCellDesc), bytes = (size_t)yuv_list_desc_bytes(route);
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
    YuvListDstDesc* host_dst = reinterpret_cast<YuvListDstDesc*>(slot.pin.data() + cell_bytes);        // (80 is a multiple of 8)
    std::vector<ListCellDesc> one;
    std::vector<YuvListDstDesc> one_dst;
    std::vector<size_t> at;                        // first entry of each pass, the same in both tables
    size_t pos = 0;
    for (const AtlasPass& p : route.passes) {
        if (!build_cell_descs(route, p, rects, nullptr, dw, dh, one) || one.back().rs_tile0 > 0x7fffffffu || one.back().rep_tile0 > 0x7fffffffu ||
            one.back().sc_tile0 > 0x7fffffffu || !build_yuv_dst_descs(route, p, rects, dsts, s.g, one_dst) || one_dst.back().ch_tile0 > 0x7fffffffu)
            return fail(SRCNN_E_UNSUPPORTED, "an atlas of %u cells has more tiles than one launch takes", p.count);
        memcpy(host + pos, one.data(), one.size() * sizeof(ListCellDesc));
        memcpy(host_dst + pos, one_dst.data(), one_dst.size() * sizeof(YuvListDstDesc));
        at.push_back(pos);
        pos += one.size();
    }
    unsigned char* dev = ws.list.data();
    HIP_TRY(hipMemcpyAsync(dev, slot.pin.data(), bytes, hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipEventRecord(slot.ev.get(), c.s));
    slot.pending = true;
    const ListCellDesc* dev_cells = reinterpret_cast<const ListCellDesc*>(dev);
    const YuvListDstDesc* dev_dst = reinterpret_cast<const YuvListDstDesc*>(dev + cell_bytes);
    for (size_t k = 0; k < route.passes.size(); ++k)
        if ((rc = list_pass(c, s, t, route.passes[k], dev_cells + at[k], dev_dst + at[k], host + at[k], host_dst + at[k]))) return rc;
    return SRCNN_OK;
}

}  // namespace

extern "C" {

int srcnn_yuv_rect_list_abi_version(void) { return SRCNN_AMD_YUV_RECT_LIST_VERSION; }

int srcnn_yuv_upscale_rect_list_plan(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                     const srcnn_yuv_rect_item* items, unsigned n, unsigned item_size, srcnn_rect_list_plan* plan)
{
    int rc;
    if (!plan) return fail(SRCNN_E_ARG, "NULL plan");
    if (plan->struct_size != sizeof(srcnn_rect_list_plan))
        return fail(SRCNN_E_ARG, "plan->struct_size %u is not sizeof(srcnn_rect_list_plan) = %zu", plan->struct_size, sizeof(srcnn_rect_list_plan));
    if ((rc = check_list(items, n, item_size))) return rc;
    srcnn_rect_list_plan out{};
    out.struct_size = (unsigned)sizeof(srcnn_rect_list_plan);
    if (n == 0) { *plan = out; return SRCNN_OK; }
    YuvGeom g;
    unsigned dw = 0, dh = 0;
    if ((rc = yuv_geom_from_format(fmt, g))) return rc;
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    std::vector<ListRect> rects(n);
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_yuv_rect_item& it = items[k];
        if ((rc = check_yuv_rect_place(g, dw, dh, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
    }
    YuvRouteInputs in = route_inputs(g, w, h, dw, dh, G.mode.load(), false);
    AxisTable th, tv, cth, ctv;
    if (may_batch(in)) {
        const int cfilter = chroma_filter(filter);
        th = build_axis_table(filter, dw, w);
        tv = build_axis_table(filter, dh, h);
        cth = build_axis_table(cfilter, g.ccols(dw), g.ccols(w));
        ctv = build_axis_table(cfilter, g.crows(dh), g.crows(h));
        in.y.th = TileAxis{th.first.data(), th.taps.data(), th.max_taps};
        in.y.tv = TileAxis{tv.first.data(), tv.taps.data(), tv.max_taps};
        in.cth = TileAxis{cth.first.data(), cth.taps.data(), cth.max_taps};
        in.ctv = TileAxis{ctv.first.data(), ctv.taps.data(), ctv.max_taps};
    }
    const RectListRoute route = route_yuv_rect_list(rects.data(), n, in);
    out.batched_items = (unsigned)route.cells.size();
    out.single_items = (unsigned)route.single.size();
    out.atlases = (unsigned)route.passes.size();
    out.cell_samples = route.cell_samples;
    out.atlas_samples = route.atlas_samples;
    out.scratch_bytes = largest_atlas(route) * (kAtlasSampleBytes + 8) + yuv_list_desc_bytes(route);
    *plan = out;
    return SRCNN_OK;
}

int srcnn_yuv_upscale_rect_list_dev(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                    const void* const src[3], const size_t src_pitch[3], const srcnn_yuv_rect_item* items, unsigned n,
                                    unsigned item_size, void* stream)
{
    int rc;
    if ((rc = check_list(items, n, item_size))) return rc;
    if (n == 0) return SRCNN_OK;
    // the frame, in the order of srcnn_yuv_upscale_rect_dev
    YuvGeom g;
    unsigned dw = 0, dh = 0;
    if ((rc = yuv_geom_from_format(fmt, g))) return rc;
    const int np = g.semi ? 2 : 3;
    if (!src) return fail(SRCNN_E_ARG, "NULL plane array");
    for (int k = 0; k < np; ++k)
        if (!src[k]) return fail(SRCNN_E_ARG, "NULL plane %d", k);
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    YuvPlane in[3];
    if ((rc = describe_yuv_side(g, w, h, src, src_pitch, "input", in))) return rc;
    // every item with the single call's per-rect rules, in its order; nothing has been queued yet
    std::vector<ListRect> rects(n);
    std::vector<YuvListDst> dsts(n);
    std::vector<YuvPlane> outs((size_t)3 * n);
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_yuv_rect_item& it = items[k];
        YuvPlane* out = outs.data() + (size_t)3 * k;
        for (int p = 0; p < np; ++p)
            if (!it.dst[p]) return fail(SRCNN_E_ARG, "item %u: NULL plane %d", k, p);
        if ((rc = check_yuv_rect_place(g, dw, dh, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        if ((rc = check_yuv_rect_planes(g, it.rw, it.rh, it.dst, it.dst_pitch, in, out))) return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
        YuvListDst& q = dsts[k];
        q = YuvListDst{};
        for (int p = 0; p < np; ++p) { q.plane[p] = it.dst[p]; q.pitch[p] = out[p].pitch; }
    }
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    Call& c = sc.c;
    // a capture that is not the library's own, as run_conv12 detects it: the descriptor upload and the tile queue stay out of it
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool foreign_capture = c.s && c.ws && !c.ws->frozen && hipStreamIsCapturing(c.s, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive;
    YuvRouteInputs ri = route_inputs(g, w, h, dw, dh, c.mode, foreign_capture);
    Tables t;
    if (may_batch(ri)) {
        const int cfilter = chroma_filter(filter);
        if ((rc = get_table(c, filter, dw, w, t.th)) || (rc = get_table(c, filter, dh, h, t.tv)) ||
            (rc = get_table(c, cfilter, g.ccols(dw), g.ccols(w), t.cth)) || (rc = get_table(c, cfilter, g.crows(dh), g.crows(h), t.ctv)))
            return rc;
        ri.y.th = TileAxis{t.th->h_first.data(), t.th->h_taps.data(), t.th->max_taps};
        ri.y.tv = TileAxis{t.tv->h_first.data(), t.tv->h_taps.data(), t.tv->max_taps};
        ri.cth = TileAxis{t.cth->h_first.data(), t.cth->h_taps.data(), t.cth->max_taps};
        ri.ctv = TileAxis{t.ctv->h_first.data(), t.ctv->h_taps.data(), t.ctv->max_taps};
    }
    const RectListRoute route = route_yuv_rect_list(rects.data(), n, ri);
    const Source s{g, in, w, h};
    if (!route.cells.empty() && (rc = list_batched(c, s, dw, dh, t, route, rects.data(), dsts.data()))) return rc;
    for (unsigned k : route.single) {
        const ListRect& r = rects[k];
        if ((rc = yuv_rect(c, g, w, h, dw, dh, filter, in, outs.data() + (size_t)3 * k, r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh))) return rc;
    }
    return SRCNN_OK;
}

}  // extern "C"
