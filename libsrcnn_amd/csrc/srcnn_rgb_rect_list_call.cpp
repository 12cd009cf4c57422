// srcnn_rgb_rect_list_call.cpp -- the RGB(A) rect LIST call (include/srcnn_amd_rgb_rect_list.h): its argument checks, the chroma
// condition of srcnn_rgb_rect_atlas.hpp on the route, and what RGB(A) adds to the list skeleton (srcnn_rect_list_call.hpp:
// the descriptor upload and the launches of an atlas): the destination table and the resample and merge of
// srcnn_rgb_rect_list.hip.  Single items go through rgb_rect of srcnn_frames.cpp, exactly as the single call runs it.
#include <vector>

#include "../../include/srcnn_amd_rgb_rect_list.h"
#include "srcnn_frame_args.hpp"
#include "srcnn_rect_list_call.hpp"
#include "srcnn_rect_source.hpp"
#include "srcnn_rgb.h"
#include "srcnn_rgb_rect_atlas.hpp"

using namespace srcnn;

namespace {

static_assert(sizeof(srcnn_rgb_rect_item) == 96 || sizeof(void*) != 8, "the header states 96 B per item on LP64");
static_assert(sizeof(ListCellDesc) == 80 && sizeof(ListDstDesc) == 88, "the header states 80 + 88 B per batched item");

int check_list(const srcnn_rgb_rect_item* items, unsigned n, unsigned item_size)
{
    return check_list_header(items, n, item_size, sizeof(srcnn_rgb_rect_item), "srcnn_rgb_rect_item");
}

RgbRouteInputs route_inputs(unsigned w, unsigned h, unsigned dw, unsigned dh, int mode, bool foreign)
{
    RgbRouteInputs in;
    in.y = list_route_inputs(w, h, dw, dh, mode, foreign || settings().rgb_rect_list_unfused);
    return in;
}
bool may_batch(const RgbRouteInputs& in) { return list_may_batch(in.y); }

// Y: (dw <- w), (dh <- h); chroma: the same axes with chroma_filter
ListAxes list_axes(int filter, unsigned w, unsigned h, unsigned dw, unsigned dh)
{
    const int cfilter = chroma_filter(filter);
    return ListAxes{{filter, dw, w}, {filter, dh, h}, {cfilter, dw, w}, {cfilter, dh, h}};
}

struct Source {
    const RgbRule& g;
    const unsigned char* src[4];
    size_t spitch[4];
    unsigned w, h;
};

// RGB(A) in the skeleton: one ListDstDesc per cell, Y' read by k_rgb_list_resample, colour resampled and merged by k_rgb_list_merge
struct Shell {
    using Dst = ListDstDesc;
    static constexpr unsigned kDstClosing = 0;
    static constexpr const char* kTrace = "srcnn rgb rect list";
    static constexpr const char* kName = "rgb_upscale_rect_list";
    const Source& s;
    const Tables& t;
    const RgbListLayout& lay;
    const RgbListDst* dsts;
    const ListOut* outs() const { return nullptr; }
    bool build_dst(const RectListRoute& route, const AtlasPass& pass, const ListRect*, std::vector<Dst>& d) const
    {
        build_dst_descs(route, pass, dsts, lay, d);
        return true;
    }
    void fill(Call& c, const ListPass<Dst>& p) const
    {
        launch_rgb_list_resample(s.g, s.src, s.spitch, s.w, s.h, t.th->view(), t.tv->view(), p.d, p.count, p.end, c.ws->up.data(), p.W, c.s);
    }
    void store(Call& c, const ListPass<Dst>& p) const
    {
        launch_rgb_list_merge(s.g, s.src, s.spitch, s.w, s.h, t.cth->view(), t.ctv->view(), p.d, p.dd, p.count, p.end, c.ws->win.data(), p.W, c.s);
    }
};

}  // namespace

extern "C" {

int srcnn_rgb_rect_list_abi_version(void) { return SRCNN_AMD_RGB_RECT_LIST_VERSION; }

int srcnn_rgb_upscale_rect_list_plan(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                     const srcnn_rgb_rect_item* items, unsigned n, unsigned item_size, srcnn_rect_list_plan* plan)
{
    int rc;
    if ((rc = check_plan(plan))) return rc;
    if ((rc = check_list(items, n, item_size))) return rc;
    if (n == 0) { fill_plan(plan, RectListRoute{}, 0); return SRCNN_OK; }
    RgbRule g;
    unsigned dw = 0, dh = 0;
    if ((rc = rgb_rule_from_format(fmt, g))) return rc;
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    std::vector<ListRect> rects(n);
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_rgb_rect_item& it = items[k];
        if ((rc = check_rect_inside(dw, dh, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
    }
    RgbRouteInputs in = route_inputs(w, h, dw, dh, G.mode.load(), false);
    PlanTables t;
    if (may_batch(in)) {
        build_tables(list_axes(filter, w, h, dw, dh), t);
        set_tile_axes(in, t);
    }
    const RectListRoute route = route_rgb_rect_list(rects.data(), n, in);
    fill_plan(plan, route, rgb_list_desc_bytes(route));
    return SRCNN_OK;
}

int srcnn_rgb_upscale_rect_list_dev(const srcnn_rgb_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                    const void* const src[4], const size_t src_pitch[4], const srcnn_rgb_rect_item* items, unsigned n,
                                    unsigned item_size, void* stream)
{
    int rc;
    if ((rc = check_list(items, n, item_size))) return rc;
    if (n == 0) return SRCNN_OK;
    // the frame, in the order of srcnn_rgb_upscale_rect_dev
    RgbRule g;
    unsigned dw = 0, dh = 0;
    if ((rc = rgb_rule_from_format(fmt, g))) return rc;
    const int np = g.planar ? g.ch : 1;
    if (!src) return fail(SRCNN_E_ARG, "NULL plane array");
    for (int k = 0; k < np; ++k)
        if (!src[k]) return fail(SRCNN_E_ARG, "NULL plane %d", k);
    if ((rc = check_scale(w, h, multiply, filter, dw, dh))) return rc;
    YuvPlane in[4];
    const RgbListLayout lay{(unsigned)g.bps, (unsigned)g.ch, g.planar};
    for (int k = 0; k < np; ++k)
        if ((rc = describe_plane(in[k], src[k], src_pitch ? src_pitch[k] : 0, lay.row_bytes(w), h, g.bps, "input", k))) return rc;
    // every item with the single call's per-rect rules, in its order; nothing has been queued yet
    std::vector<ListRect> rects(n);
    std::vector<RgbListDst> dsts(n);
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_rgb_rect_item& it = items[k];
        YuvPlane again[4], out[5], conv;
        for (int p = 0; p < np; ++p)
            if (!it.dst[p]) return fail(SRCNN_E_ARG, "item %u: NULL plane %d", k, p);
        if ((rc = check_rect_inside(dw, dh, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        if ((rc = describe_rgb_planes(g, w, h, it.rw, it.rh, src, src_pitch, it.dst, it.dst_pitch, it.dst_conv, it.dst_conv_pitch, again, out, conv)))
            return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
        RgbListDst& q = dsts[k];
        q = RgbListDst{};
        for (int p = 0; p < np; ++p) { q.plane[p] = it.dst[p]; q.pitch[p] = out[p].pitch; }
        q.conv = it.dst_conv;
        q.conv_pitch = it.dst_conv ? conv.pitch : 0;
    }
    StreamCall sc(stream);
    if (sc.rc) return sc.rc;
    Call& c = sc.c;
    RgbRouteInputs ri = route_inputs(w, h, dw, dh, c.mode, foreign_capture(c));
    Tables t;
    if (may_batch(ri)) {
        if ((rc = get_tables(c, list_axes(filter, w, h, dw, dh), t))) return rc;
        set_tile_axes(ri, t);
    }
    const RectListRoute route = route_rgb_rect_list(rects.data(), n, ri);
    Source s{g, {nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0}, w, h};
    for (int k = 0; k < np; ++k) { s.src[k] = in[k].lo; s.spitch[k] = in[k].pitch; }
    const Shell sh{s, t, lay, dsts.data()};
    if (!route.cells.empty() && (rc = list_batched(c, sh, dw, dh, route, rects.data()))) return rc;
    for (unsigned k : route.single) {
        const ListRect& r = rects[k];
        const RgbListDst& q = dsts[k];
        YuvPlane out[4], conv;
        for (int p = 0; p < np; ++p) {
            out[p].lo = static_cast<const unsigned char*>(q.plane[p]);
            out[p].pitch = q.pitch[p]; out[p].row_bytes = lay.row_bytes(r.rw); out[p].rows = r.rh;
        }
        if (q.conv) {
            conv.lo = static_cast<const unsigned char*>(q.conv);
            conv.pitch = q.conv_pitch; conv.row_bytes = (size_t)g.bps * r.rw; conv.rows = r.rh;
        }
        if ((rc = rgb_rect(c, g, w, h, dw, dh, filter, in, out, conv, r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh))) return rc;
    }
    return SRCNN_OK;
}

}  // extern "C"
