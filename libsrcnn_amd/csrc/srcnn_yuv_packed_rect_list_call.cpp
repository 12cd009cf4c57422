// srcnn_yuv_packed_rect_list_call.cpp -- the packed YUV rect LIST call (include/srcnn_amd_yuv_packed_rect_list.h): its argument
// checks, the chroma condition of srcnn_yuv_packed_rect_atlas.hpp on the route, and what the packed formats add to the list
// skeleton (srcnn_rect_list_call.hpp: the descriptor upload and the launches of an atlas): the destination table with its
// chroma tile totals, and the luma resample and the merge of srcnn_yuv_packed_rect_list.hip.  Single items go through
// yuv_packed_rect of srcnn_frames.cpp, exactly as the single call runs it.
#include <vector>

#include "../../include/srcnn_amd_yuv_packed_rect_list.h"
#include "srcnn_frame_args.hpp"
#include "srcnn_rect_list_call.hpp"
#include "srcnn_rect_source.hpp"
#include "srcnn_yuv.h"
#include "srcnn_yuv_packed_rect_atlas.hpp"

using namespace srcnn;

namespace {

static_assert(sizeof(srcnn_yuv_packed_rect_item) == 32 || sizeof(void*) != 8, "the header states 32 B per item on LP64");
static_assert(sizeof(ListCellDesc) == 80 && sizeof(YuvPackedListDstDesc) == 64, "the header states 80 + 64 B per batched item");

int check_list(const srcnn_yuv_packed_rect_item* items, unsigned n, unsigned item_size)
{
    return check_list_header(items, n, item_size, sizeof(srcnn_yuv_packed_rect_item), "srcnn_yuv_packed_rect_item");
}

YuvPackedRouteInputs route_inputs(int kind, unsigned w, unsigned h, unsigned dw, unsigned dh, int mode, bool foreign)
{
    YuvPackedRouteInputs in;
    in.kind = kind;
    in.y = list_route_inputs(w, h, dw, dh, mode, foreign || settings().yuv_packed_rect_list_unfused);
    return in;
}
bool may_batch(const YuvPackedRouteInputs& in) { return list_may_batch(in.y) && in.chroma_grows(); }

// Y: (dw <- w), (dh <- h); chroma: (dcw <- cw), (dh <- h) with chroma_filter
ListAxes list_axes(const YuvPackedGeom& g, int filter, unsigned w, unsigned h, unsigned dw, unsigned dh)
{
    const int cfilter = chroma_filter(filter);
    return ListAxes{{filter, dw, w}, {filter, dh, h}, {cfilter, g.ccols(dw), g.ccols(w)}, {cfilter, dh, h}};
}

struct Source {
    const YuvPackedGeom& g;
    const YuvPlane& in;                              // the WHOLE frame
    unsigned w, h;
};

// Packed YUV in the skeleton: one YuvPackedListDstDesc per cell and a closing one, luma read by k_yuvp_list_resample, chroma /
// alpha resampled, merged with Y' and stored by k_yuvp_list_merge
struct Shell {
    using Dst = YuvPackedListDstDesc;
    static constexpr unsigned kDstClosing = 1;
    static constexpr const char* kTrace = "srcnn yuv packed rect list";
    static constexpr const char* kName = "yuv_packed_upscale_rect_list";
    const Source& s;
    const Tables& t;
    const TileAxis& cth;                             // the host copy of t.cth (the route's inputs have it)
    unsigned dw;
    const YuvPackedListDst* dsts;
    const ListOut* outs() const { return nullptr; }
    bool build_dst(const RectListRoute& route, const AtlasPass& pass, const ListRect* rects, std::vector<Dst>& d) const
    {
        return build_yuv_packed_dst_descs(route, pass, rects, dsts, s.g.rule.kind, s.w, dw, cth, d);
    }
    void fill(Call& c, const ListPass<Dst>& p) const
    {
        launch_yuvp_list_resample(s.g.rule, s.in.lo, s.in.pitch, s.w, s.h, t.th->view(), t.tv->view(), p.d, p.count, p.end, c.ws->up.data(), p.W, c.s);
    }
    void store(Call& c, const ListPass<Dst>& p) const
    {
        launch_yuvp_list_merge(s.g.rule, s.in.lo, s.in.pitch, s.w, s.h, t.cth->view(), t.ctv->view(), p.d, p.dd, p.count, p.hdd[p.count], c.ws->win.data(),
                               p.W, c.s);
    }
};

}  // namespace

extern "C" {

int srcnn_yuv_packed_rect_list_abi_version(void) { return SRCNN_AMD_YUV_PACKED_RECT_LIST_VERSION; }

int srcnn_yuv_packed_upscale_rect_list_plan(int format, unsigned w, unsigned h, float multiply, int filter, const srcnn_yuv_packed_rect_item* items,
                                            unsigned n, unsigned item_size, srcnn_rect_list_plan* plan)
{
    int rc;
    if ((rc = check_plan(plan))) return rc;
    if ((rc = check_list(items, n, item_size))) return rc;
    if (n == 0) { fill_plan(plan, RectListRoute{}, 0); return SRCNN_OK; }
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
    PlanTables t;
    if (may_batch(in)) {
        build_tables(list_axes(g, filter, w, h, dw, dh), t);
        set_tile_axes(in, t);
    }
    const RectListRoute route = route_yuv_packed_rect_list(rects.data(), n, in);
    fill_plan(plan, route, yuv_packed_list_desc_bytes(route));
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
    YuvPackedRouteInputs ri = route_inputs(g.rule.kind, w, h, dw, dh, c.mode, foreign_capture(c));
    Tables t;
    if (may_batch(ri)) {
        if ((rc = get_tables(c, list_axes(g, filter, w, h, dw, dh), t))) return rc;
        set_tile_axes(ri, t);
    }
    const RectListRoute route = route_yuv_packed_rect_list(rects.data(), n, ri);
    const Source s{g, in, w, h};
    const Shell sh{s, t, ri.cth, dw, dsts.data()};
    if (!route.cells.empty() && (rc = list_batched(c, sh, dw, dh, route, rects.data()))) return rc;
    for (unsigned k : route.single) {
        const ListRect& r = rects[k];
        if ((rc = yuv_packed_rect(c, g, w, h, dw, dh, filter, in, outs[k], r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh))) return rc;
    }
    return SRCNN_OK;
}

}  // extern "C"
