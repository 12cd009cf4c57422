// srcnn_rect_list_call.hpp -- the host skeleton under the four rect LIST calls (Y plane: srcnn_rect_list_call.cpp, RGB(A):
// srcnn_rgb_rect_list_call.cpp, planar / semi-planar YUV: srcnn_yuv_rect_list_call.cpp, packed YUV:
// srcnn_yuv_packed_rect_list_call.cpp).  What a list call is whatever its surface: the checks of the list header, the plan
// structure, the common route inputs, the four resampling tables, the probe for a caller's capture, and the batched route
// (list_batched below) with its staging-slot protocol and the launches of an atlas.  A surface adds a "shell": its destination
// table and the launches that read the source into the atlas and store the result.  Internal.
#pragma once
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/srcnn_amd_rect_list.h"
#include "resample_table.hpp"
#include "srcnn_host.hpp"
#include "srcnn_rect_atlas.hpp"
#include "srcnn_rect_list.h"

namespace srcnn {

// ---- the list ----------------------------------------------------------------------------------------------------------------
// the failure of item k, with the index in front of what the single call would have said
inline int fail_item(int rc, unsigned k)
{
    const std::string why = last_error();
    return fail(rc, "item %u: %s", k, why.c_str());
}

// What both entry points of a surface refuse about the list itself, before they look at the frame or at an item.  SRCNN_OK with
// n == 0: nothing to do.
inline int check_list_header(const void* items, unsigned n, unsigned item_size, size_t item_bytes, const char* item_type)
{
    if (item_size != item_bytes) return fail(SRCNN_E_ARG, "item_size %u is not sizeof(%s) = %zu", item_size, item_type, item_bytes);
    if (n == 0) return SRCNN_OK;
    if (!items) return fail(SRCNN_E_ARG, "NULL items with n = %u", n);
    if (n > kRectListMax) return fail(SRCNN_E_UNSUPPORTED, "%u items: a list holds at most %u", n, kRectListMax);
    return SRCNN_OK;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------
inline int check_plan(const srcnn_rect_list_plan* plan)
{
    if (!plan) return fail(SRCNN_E_ARG, "NULL plan");
    if (plan->struct_size != sizeof(srcnn_rect_list_plan))
        return fail(SRCNN_E_ARG, "plan->struct_size %u is not sizeof(srcnn_rect_list_plan) = %zu", plan->struct_size, sizeof(srcnn_rect_list_plan));
    return SRCNN_OK;
}

inline unsigned long long largest_atlas(const RectListRoute& route)
{
    unsigned long long largest = 0;
    for (const AtlasPass& p : route.passes) largest = std::max(largest, (unsigned long long)p.W * p.H);
    return largest;
}

// desc_bytes: the surface's descriptor tables of this route (an empty route, 0: the plan of an empty list)
inline void fill_plan(srcnn_rect_list_plan* plan, const RectListRoute& route, unsigned long long desc_bytes)
{
    srcnn_rect_list_plan out{};
    out.struct_size = (unsigned)sizeof(srcnn_rect_list_plan);
    out.batched_items = (unsigned)route.cells.size();
    out.single_items = (unsigned)route.single.size();
    out.atlases = (unsigned)route.passes.size();
    out.cell_samples = route.cell_samples;
    out.atlas_samples = route.atlas_samples;
    out.scratch_bytes = largest_atlas(route) * (kAtlasSampleBytes + 8) + desc_bytes;
    *plan = out;
}

// ---- the route's inputs ------------------------------------------------------------------------------------------------------
// unfused: the surface's own switch (SRCNN_*RECT_LIST_UNFUSED), or a stream in a foreign capture
inline RouteInputs list_route_inputs(unsigned w, unsigned h, unsigned dw, unsigned dh, int mode, bool unfused)
{
    RouteInputs in;
    in.w = w; in.h = h; in.dw = dw; in.dh = dh;
    in.strict = mode == SRCNN_MODE_STRICT;
    in.unfused = unfused;
    in.cap_bytes = G.ws_budget.load();
    in.single_samples = settings().rect_list_single_samples > 0 ? (unsigned long long)settings().rect_list_single_samples : 0;
    return in;
}
// whether any item can be batched, i.e. whether the tables are worth having (a surface with chroma adds chroma_grows())
inline bool list_may_batch(const RouteInputs& in) { return in.strict && !in.unfused && in.dw > in.w && in.dh > in.h; }

// a capture that is not the library's own, as run_conv12 detects it: the descriptor upload and the tile queue stay out of it
inline bool foreign_capture(Call& c)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return c.s && c.ws && !c.ws->frozen && hipStreamIsCapturing(c.s, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive;
}

// ---- the tables --------------------------------------------------------------------------------------------------------------
inline TileAxis tile_axis(const AxisTable& t) { return TileAxis{t.first.data(), t.taps.data(), t.max_taps}; }                // the plan calls: no device
inline TileAxis tile_axis(const TableRef& t) { return TileAxis{t->h_first.data(), t->h_taps.data(), t->max_taps}; }          // the device calls: the cache

struct AxisSpec { int filter; unsigned dst_len, src_len; };
struct ListAxes { AxisSpec th, tv, cth, ctv; };        // what a colour surface says about its tables: Y, then chroma with chroma_filter
struct PlanTables { AxisTable th, tv, cth, ctv; };
struct Tables { TableRef th, tv, cth, ctv; };

inline AxisTable build_axis_table(const AxisSpec& a) { return build_axis_table(a.filter, a.dst_len, a.src_len); }
inline void build_tables(const ListAxes& a, PlanTables& t)
{
    t.th = build_axis_table(a.th); t.tv = build_axis_table(a.tv); t.cth = build_axis_table(a.cth); t.ctv = build_axis_table(a.ctv);
}
inline int get_table(Call& c, const AxisSpec& a, TableRef& out) { return get_table(c, a.filter, a.dst_len, a.src_len, out); }
inline int get_tables(Call& c, const ListAxes& a, Tables& t)
{
    int rc;
    if ((rc = get_table(c, a.th, t.th)) || (rc = get_table(c, a.tv, t.tv)) || (rc = get_table(c, a.cth, t.cth)) || (rc = get_table(c, a.ctv, t.ctv))) return rc;
    return SRCNN_OK;
}
// T: PlanTables or Tables; In: a colour surface's route inputs (the Y list's in `y`, the chroma axes beside it)
template <class T, class In>
void set_tile_axes(In& in, const T& t)
{
    in.y.th = tile_axis(t.th); in.y.tv = tile_axis(t.tv);
    in.cth = tile_axis(t.cth); in.ctv = tile_axis(t.ctv);
}

// ---- the batched route -------------------------------------------------------------------------------------------------------
struct NoDst {};        // Shell::Dst of a surface without a destination table (the Y list: ListCellDesc carries d_out)

// One pass as the shell's launches see it.  d / dd: the device copies of the pass's cell and destination tables; `end` / hdd:
// the closing cell entry (the tile totals) and the destination table on the host.
template <class Dst>
struct ListPass {
    unsigned count, W;                  // cells, floats per row of the atlas planes
    const ListCellDesc* d;
    const ListCellDesc& end;
    const Dst* dd;
    const Dst* hdd;
};

// The batched route of every surface.  The cell tables of every pass, then the destination tables of every pass
// (ListTableLayout, srcnn_rect_atlas.hpp), go to the device in ONE copy, in stream order, from a page-locked slot that belongs
// to this call until its event has passed (ListStaging, srcnn_host.hpp); then the passes, one after another, each the launches
// of an atlas: the shell's fill, replicate to depth 6, layers 1+2, replicate to depth 2 over the 32 planes, layer 3, the
// shell's store.
//
// A Shell has
//   Dst                    the entry of its destination table, or NoDst
//   kDstClosing            1: that table has a closing entry per pass whose ch_tile0 is a tile total; 0: count entries
//   kTrace, kName          the trace label and the name in the SRCNN_E_HIP message
//   outs()                 what build_cell_descs takes for `out` (the Y list's destinations; otherwise NULL)
//   build_dst(route, pass, rects, v)     one pass's destination table into v; false: a total does not fit 32 bits
//   fill(c, p)             the launch that resamples the source's luma into ws.up (inside the RESAMPLE timer)
//   store(c, p)            the launch(es) that take the result out of ws.win (outside the timers)
template <class Shell>
int list_batched(Call& c, const Shell& sh, unsigned dw, unsigned dh, const RectListRoute& route, const ListRect* rects)
{
    using Dst = typename Shell::Dst;
    constexpr bool kHasDst = !std::is_same<Dst, NoDst>::value;
    Workspace& ws = *c.ws;
    int rc;
    const ListTableLayout lay(route, kHasDst ? sizeof(Dst) : 0, Shell::kDstClosing);
    // all scratch first: growing drains the device, which nothing queued below may see half way
    const size_t largest = (size_t)largest_atlas(route);
    if ((rc = ws.grow(ws.up, largest)) || (rc = ws.grow(ws.win, largest)) || (rc = ws.grow(ws.c2, (size_t)C2N * largest)) || (rc = ws.grow(ws.list, lay.bytes))) return rc;
    ListStaging::Slot& slot = ws.list_stage.slot[ws.list_stage.next];
    ws.list_stage.next = (ws.list_stage.next + 1) % ListStaging::kSlots;
    if (slot.pending) {
        if (wait_event(slot.ev.get()) != hipSuccess) return fail(SRCNN_E_HIP, "an earlier descriptor upload of this stream failed");
        slot.pending = false;
    }
    if ((rc = slot.pin.grow(lay.bytes, *c.cx))) return rc;
    if (!slot.ev) HIP_TRY(hipEventCreateWithFlags(slot.ev.put(), hipEventDisableTiming));
    unsigned char* host = slot.pin.data();
    std::vector<ListCellDesc> one;
    std::vector<Dst> one_dst;
    for (size_t k = 0; k < route.passes.size(); ++k) {
        const AtlasPass& p = route.passes[k];
        bool fits = build_cell_descs(route, p, rects, sh.outs(), dw, dh, one) && one.back().rs_tile0 <= 0x7fffffffu && one.back().rep_tile0 <= 0x7fffffffu &&
                    one.back().sc_tile0 <= 0x7fffffffu && sh.build_dst(route, p, rects, one_dst);
        if constexpr (Shell::kDstClosing != 0) fits = fits && one_dst.back().ch_tile0 <= 0x7fffffffu;
        if (!fits) return fail(SRCNN_E_UNSUPPORTED, "an atlas of %u cells has more tiles than one launch takes", p.count);
        std::copy(one.begin(), one.end(), lay.cells(host, route, k));
        if constexpr (kHasDst) std::copy(one_dst.begin(), one_dst.end(), lay.template dsts<Dst>(host, route, k));
    }
    unsigned char* dev = ws.list.data();
    HIP_TRY(hipMemcpyAsync(dev, host, lay.bytes, hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipEventRecord(slot.ev.get(), c.s));
    slot.pending = true;
    for (size_t k = 0; k < route.passes.size(); ++k) {
        const AtlasPass& pass = route.passes[k];
        const unsigned W = pass.W, H = pass.H;
        const size_t plane = (size_t)W * H;
        const ListCellDesc* d = lay.cells(dev, route, k);
        const ListCellDesc& end = lay.cells(host, route, k)[pass.count];
        const Dst* dd = kHasDst ? lay.template dsts<Dst>(dev, route, k) : nullptr;
        const Dst* hdd = kHasDst ? lay.template dsts<Dst>(host, route, k) : nullptr;
        const ListPass<Dst> p{pass.count, W, d, end, dd, hdd};
        TraceRange tr("%s atlas %ux%u, %u cells", Shell::kTrace, W, H, pass.count);
        {
            StageTimer t(SRCNN_STAGE_RESAMPLE, c);
            sh.fill(c, p);
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
            launch_conv3(ws.c2.data(), plane, (int)W, (int)H, 0, (int)H, ws.win.data(), 0, (int)H, c.relax(), c.s);
        }
        sh.store(c, p);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
            ws.queue_dirty = true;
            return fail(SRCNN_E_HIP, "%s: %s", Shell::kName, hipGetErrorString(e));
        }
    }
    return SRCNN_OK;
}

}  // namespace srcnn
