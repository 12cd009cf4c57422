// srcnn_rect_list_call.cpp -- the rect LIST call (include/srcnn_amd_rect_list.h): argument checks, routing and packing
// (srcnn_rect_atlas.hpp), the descriptor upload and the six launches of an atlas (srcnn_rect_list.hip around the unchanged layer
// kernels).  Single items go through y_path_rect of srcnn_capi.cpp, exactly as the single call runs it.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/srcnn_amd_rect.h"
#include "../../include/srcnn_amd_rect_list.h"
#include "resample_table.hpp"
#include "srcnn_frame_args.hpp"
#include "srcnn_host.hpp"
#include "srcnn_rect_atlas.hpp"
#include "srcnn_rect_list.h"

using namespace srcnn;

// ---- a list of rectangles of the output (include/srcnn_amd_rect_list.h) ---------------------------
namespace {

static_assert(sizeof(ListCellDesc) == 80, "the header states 80 B per batched item");

// the failure of item k, with the index in front of what the single call would have said
int fail_item(int rc, unsigned k)
{
    const std::string why = last_error();
    return fail(rc, "item %u: %s", k, why.c_str());
}

// What both list entry points refuse before they look at an item.  SRCNN_OK with n == 0: nothing to do.
int check_rect_list_frame(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const srcnn_rect_item* items, unsigned n, unsigned item_size)
{
    if (item_size != sizeof(srcnn_rect_item)) return fail(SRCNN_E_ARG, "item_size %u is not sizeof(srcnn_rect_item) = %zu", item_size, sizeof(srcnn_rect_item));
    if (n == 0) return SRCNN_OK;
    if (!items) return fail(SRCNN_E_ARG, "NULL items with n = %u", n);
    if (n > kRectListMax) return fail(SRCNN_E_UNSUPPORTED, "%u items: a list holds at most %u", n, kRectListMax);
    if (w == 0 || h == 0) return fail(SRCNN_E_ARG, "zero dimension (%ux%u)", w, h);
    if (dw == 0 || dh == 0) return fail(SRCNN_E_SCALE, "scaled size %ux%u", dw, dh);
    if (filter < 0 || filter > 4) return fail(SRCNN_E_ARG, "bad filter %d", filter);
    return SRCNN_OK;
}

RouteInputs rect_list_inputs(unsigned w, unsigned h, unsigned dw, unsigned dh, int mode, bool unfused)
{
    RouteInputs in;
    in.w = w; in.h = h; in.dw = dw; in.dh = dh;
    in.strict = mode == SRCNN_MODE_STRICT;
    in.unfused = unfused || settings().rect_list_unfused;
    in.cap_bytes = G.ws_budget.load();
    in.single_samples = settings().rect_list_single_samples > 0 ? (unsigned long long)settings().rect_list_single_samples : 0;
    return in;
}
bool rect_list_may_batch(const RouteInputs& in) { return in.strict && !in.unfused && in.dw > in.w && in.dh > in.h; }

size_t rect_list_desc_entries(const RectListRoute& route) { return route.cells.size() + route.passes.size(); }

// One atlas: the six launches.  d: the device copy of the pass's descriptor table, hd: the host copy.
int rect_list_pass(Call& c, const float* d_in, size_t in_stride, unsigned w, unsigned h, const TableRef& th, const TableRef& tv,
                   const AtlasPass& pass, const ListCellDesc* d, const ListCellDesc* hd)
{
    Workspace& ws = *c.ws;
    const ListCellDesc& end = hd[pass.count];
    const unsigned W = pass.W, H = pass.H;
    const size_t plane = (size_t)W * H;
    TraceRange tr("srcnn rect list atlas %ux%u, %u cells", W, H, pass.count);
    {
        StageTimer t(SRCNN_STAGE_RESAMPLE, c);
        launch_list_resample(d_in, in_stride, w, h, th->view(), tv->view(), d, pass.count, end, ws.up.data(), W, c.s);
        launch_list_replicate(d, pass.count, end, ws.up.data(), W, 0, 1, kCellMargin, c.s);
    }
    {
        StageTimer t(SRCNN_STAGE_CONV12, c);
        run_conv12(c, ws.up.data(), (int)W, (int)H, 0, (int)H, ws.c2.data(), plane, 0, (int)H);
    }
    {
        StageTimer t(SRCNN_STAGE_CONV3, c);
        // layer 3 clamps the ACTIVATIONS to the plane's edge: the ring of 2 around a rect that lies outside the plane gets the
        // activation at the clamped coordinate (layer 2 over the replicated input above is not that)
        launch_list_replicate(d, pass.count, end, ws.c2.data(), W, plane, C2N, 2, c.s);
        launch_layer3(ws.c2.data(), plane, (int)W, (int)H, 0, (int)H, ws.win.data(), 0, (int)H, c.relax(), c.s);
    }
    launch_list_scatter(d, pass.count, end, ws.win.data(), W, c.s);      // (outside the stage timers)
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
        ws.queue_dirty = true;
        return fail(SRCNN_E_HIP, "y_path_rect_list: %s", hipGetErrorString(e));
    }
    return SRCNN_OK;
}

// The batched route: every pass's descriptor table goes to the device in ONE copy, in stream order, from a page-locked slot
// that belongs to this call until its event has passed (ListStaging, srcnn_host.hpp); then the passes, one after another.
int rect_list_batched(Call& c, const float* d_in, size_t in_stride, unsigned w, unsigned h, unsigned dw, unsigned dh, const TableRef& th,
                      const TableRef& tv, const RectListRoute& route, const ListRect* rects, const ListOut* outs)
{
    Workspace& ws = *c.ws;
    int rc;
    const size_t entries = rect_list_desc_entries(route), bytes = entries * sizeof(ListCellDesc);
    // all scratch first: growing drains the device, which nothing queued below may see half way
    size_t largest = 0;
    for (const AtlasPass& p : route.passes) largest = std::max(largest, (size_t)p.W * p.H);
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
    std::vector<ListCellDesc> one;
    std::vector<size_t> at;                        // first entry of each pass
    size_t pos = 0;
    for (const AtlasPass& p : route.passes) {
        if (!build_cell_descs(route, p, rects, outs, dw, dh, one) || one.back().rs_tile0 > 0x7fffffffu || one.back().rep_tile0 > 0x7fffffffu ||
            one.back().sc_tile0 > 0x7fffffffu)
            return fail(SRCNN_E_UNSUPPORTED, "an atlas of %u cells has more tiles than one launch takes", p.count);
        memcpy(host + pos, one.data(), one.size() * sizeof(ListCellDesc));
        at.push_back(pos);
        pos += one.size();
    }
    ListCellDesc* dev = reinterpret_cast<ListCellDesc*>(ws.list.data());
    HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipEventRecord(slot.ev.get(), c.s));
    slot.pending = true;
    for (size_t k = 0; k < route.passes.size(); ++k)
        if ((rc = rect_list_pass(c, d_in, in_stride, w, h, th, tv, route.passes[k], dev + at[k], host + at[k]))) return rc;
    return SRCNN_OK;
}

}  // namespace

extern "C" {

int srcnn_rect_list_abi_version(void) { return SRCNN_AMD_RECT_LIST_VERSION; }

int srcnn_y_path_rect_list_plan(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const srcnn_rect_item* items, unsigned n,
                                unsigned item_size, srcnn_rect_list_plan* plan)
{
    int rc;
    if (!plan) return fail(SRCNN_E_ARG, "NULL plan");
    if (plan->struct_size != sizeof(srcnn_rect_list_plan))
        return fail(SRCNN_E_ARG, "plan->struct_size %u is not sizeof(srcnn_rect_list_plan) = %zu", plan->struct_size, sizeof(srcnn_rect_list_plan));
    if ((rc = check_rect_list_frame(w, h, dw, dh, filter, items, n, item_size))) return rc;
    srcnn_rect_list_plan out{};
    out.struct_size = (unsigned)sizeof(srcnn_rect_list_plan);
    if (n == 0) { *plan = out; return SRCNN_OK; }
    std::vector<ListRect> rects(n);
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_rect_item& it = items[k];
        if ((rc = check_rect_geometry(w, h, dw, dh, filter, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        if ((rc = check_rect_limits(w, h, dw, dh, it.rh))) return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
    }
    RouteInputs in = rect_list_inputs(w, h, dw, dh, G.mode.load(), false);
    AxisTable th, tv;
    if (rect_list_may_batch(in)) {
        th = build_axis_table(filter, dw, w);
        tv = build_axis_table(filter, dh, h);
        in.th = TileAxis{th.first.data(), th.taps.data(), th.max_taps};
        in.tv = TileAxis{tv.first.data(), tv.taps.data(), tv.max_taps};
    }
    const RectListRoute route = route_rect_list(rects.data(), n, in);
    out.batched_items = (unsigned)route.cells.size();
    out.single_items = (unsigned)route.single.size();
    out.atlases = (unsigned)route.passes.size();
    out.cell_samples = route.cell_samples;
    out.atlas_samples = route.atlas_samples;
    unsigned long long largest = 0;
    for (const AtlasPass& p : route.passes) largest = std::max(largest, (unsigned long long)p.W * p.H);
    out.scratch_bytes = largest * (kAtlasSampleBytes + 8) + (unsigned long long)rect_list_desc_entries(route) * sizeof(ListCellDesc);
    *plan = out;
    return SRCNN_OK;
}

int srcnn_y_path_rect_list_f32_dev(const float* d_in, size_t in_pitch, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter,
                                   const srcnn_rect_item* items, unsigned n, unsigned item_size, void* stream)
{
    int rc;
    if ((rc = check_rect_list_frame(w, h, dw, dh, filter, items, n, item_size))) return rc;
    if (n == 0) return SRCNN_OK;
    if (!d_in) return fail(SRCNN_E_ARG, "NULL d_in");
    YuvPlane in;
    if ((rc = describe_plane(in, d_in, in_pitch, sizeof(float) * (size_t)w, h, 4, "input", 0))) return rc;
    std::vector<ListRect> rects(n);
    std::vector<ListOut> outs(n);
    for (unsigned k = 0; k < n; ++k) {              // the single call's rules, in its order; nothing has been queued yet
        const srcnn_rect_item& it = items[k];
        YuvPlane out;
        if (!it.d_out) return fail(SRCNN_E_ARG, "item %u: NULL d_out", k);
        if ((rc = check_rect_geometry(w, h, dw, dh, filter, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        if ((rc = describe_plane(out, it.d_out, it.out_pitch, sizeof(float) * (size_t)it.rw, it.rh, 4, "output", 0))) return fail_item(rc, k);
        if ((rc = check_rect_limits(w, h, dw, dh, it.rh))) return fail_item(rc, k);
        if ((rc = check_in_out_overlap(&in, 1, &out, 1))) return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
        outs[k] = ListOut{it.d_out, out.pitch / sizeof(float)};
    }
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    Call& c = sc.c;
    // a capture that is not the library's own, as run_conv12 detects it: the descriptor upload and the tile queue stay out of it
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool foreign_capture = c.s && c.ws && !c.ws->frozen && hipStreamIsCapturing(c.s, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive;
    RouteInputs ri = rect_list_inputs(w, h, dw, dh, c.mode, foreign_capture);
    TableRef th, tv;
    if (rect_list_may_batch(ri)) {
        if ((rc = get_table(c, filter, dw, w, th))) return rc;
        if ((rc = get_table(c, filter, dh, h, tv))) return rc;
        ri.th = TileAxis{th->h_first.data(), th->h_taps.data(), th->max_taps};
        ri.tv = TileAxis{tv->h_first.data(), tv->h_taps.data(), tv->max_taps};
    }
    const RectListRoute route = route_rect_list(rects.data(), n, ri);
    const size_t in_stride = in.pitch / sizeof(float);
    if (!route.cells.empty() && (rc = rect_list_batched(c, d_in, in_stride, w, h, dw, dh, th, tv, route, rects.data(), outs.data()))) return rc;
    for (unsigned k : route.single) {
        const ListRect& r = rects[k];
        if ((rc = y_path_rect(c, d_in, in_stride, 0, 0, w, h, dw, dh, filter, r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh, static_cast<float*>(outs[k].d_out), outs[k].out_stride)))
            return rc;
    }
    return SRCNN_OK;
}

}  // extern "C"
