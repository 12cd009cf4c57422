// srcnn_yuv_rect_list_call.cpp -- the planar / semi-planar YUV rect LIST call (include/srcnn_amd_yuv_rect_list.h): its argument
// checks, the chroma condition of srcnn_yuv_rect_atlas.hpp on the route, and what these formats add to the list skeleton
// (srcnn_rect_list_call.hpp: the descriptor upload and the launches of an atlas): the destination table with its chroma tile
// totals, and the luma resample, luma store and chroma launches of srcnn_yuv_rect_list.hip.  Single items go through yuv_rect
// of srcnn_frames.cpp, exactly as the single call runs it.
#include <vector>

#include "../../include/srcnn_amd_yuv_rect_list.h"
#include "srcnn_frame_args.hpp"
#include "srcnn_rect_list_call.hpp"
#include "srcnn_rect_source.hpp"
#include "srcnn_yuv.h"
#include "srcnn_yuv_rect_atlas.hpp"

using namespace srcnn;

namespace {

static_assert(sizeof(srcnn_yuv_rect_item) == 64 || sizeof(void*) != 8, "the header states 64 B per item on LP64");
static_assert(sizeof(ListCellDesc) == 80 && sizeof(YuvListDstDesc) == 80, "the header states 80 + 80 B per batched item");

int check_list(const srcnn_yuv_rect_item* items, unsigned n, unsigned item_size)
{
    return check_list_header(items, n, item_size, sizeof(srcnn_yuv_rect_item), "srcnn_yuv_rect_item");
}

YuvRouteInputs route_inputs(const YuvGeom& g, unsigned w, unsigned h, unsigned dw, unsigned dh, int mode, bool foreign)
{
    YuvRouteInputs in;
    in.g = g;
    in.y = list_route_inputs(w, h, dw, dh, mode, foreign || settings().yuv_rect_list_unfused);
    return in;
}
bool may_batch(const YuvRouteInputs& in) { return list_may_batch(in.y) && in.chroma_grows(); }

// Y: (dw <- w), (dh <- h); chroma: (dcw <- cw), (dch <- ch) with chroma_filter
ListAxes list_axes(const YuvGeom& g, int filter, unsigned w, unsigned h, unsigned dw, unsigned dh)
{
    const int cfilter = chroma_filter(filter);
    return ListAxes{{filter, dw, w}, {filter, dh, h}, {cfilter, g.ccols(dw), g.ccols(w)}, {cfilter, g.crows(dh), g.crows(h)}};
}

struct Source {
    const YuvGeom& g;
    const YuvPlane* in;                              // the WHOLE frame's planes
    unsigned w, h;
};

// Planar / semi-planar YUV in the skeleton: one YuvListDstDesc per cell and a closing one, luma read by k_yuv_list_resample and
// stored by k_yuv_list_luma, chroma resampled and stored by k_yuv_list_chroma
struct Shell {
    using Dst = YuvListDstDesc;
    static constexpr unsigned kDstClosing = 1;
    static constexpr const char* kTrace = "srcnn yuv rect list";
    static constexpr const char* kName = "yuv_upscale_rect_list";
    const Source& s;
    const Tables& t;
    const YuvListDst* dsts;
    const Yuv16Rule* rule() const { return s.g.bps == 2 ? &s.g.rule : nullptr; }
    const ListOut* outs() const { return nullptr; }
    bool build_dst(const RectListRoute& route, const AtlasPass& pass, const ListRect* rects, std::vector<Dst>& d) const
    {
        return build_yuv_dst_descs(route, pass, rects, dsts, s.g, d);
    }
    void fill(Call& c, const ListPass<Dst>& p) const
    {
        launch_yuv_list_resample(s.in[0].lo, s.in[0].pitch, s.w, s.h, rule(), t.th->view(), t.tv->view(), p.d, p.count, p.end, c.ws->up.data(), p.W, c.s);
    }
    void store(Call& c, const ListPass<Dst>& p) const
    {
        launch_yuv_list_luma(rule(), p.d, p.dd, p.count, p.end, c.ws->win.data(), p.W, c.s);
        const unsigned char* csrc[2] = {s.in[1].lo, s.in[2].lo};
        const size_t cspitch[2] = {s.in[1].pitch, s.in[2].pitch};
        launch_yuv_list_chroma(csrc, cspitch, s.g.ccols(s.w), s.g.crows(s.h), s.g.semi, rule(), t.cth->view(), t.ctv->view(), p.dd, p.count, p.hdd[p.count], c.s);
    }
};

}  // namespace

extern "C" {

int srcnn_yuv_rect_list_abi_version(void) { return SRCNN_AMD_YUV_RECT_LIST_VERSION; }

int srcnn_yuv_upscale_rect_list_plan(const srcnn_yuv_format* fmt, unsigned w, unsigned h, float multiply, int filter,
                                     const srcnn_yuv_rect_item* items, unsigned n, unsigned item_size, srcnn_rect_list_plan* plan)
{
    int rc;
    if ((rc = check_plan(plan))) return rc;
    if ((rc = check_list(items, n, item_size))) return rc;
    if (n == 0) { fill_plan(plan, RectListRoute{}, 0); return SRCNN_OK; }
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
    PlanTables t;
    if (may_batch(in)) {
        build_tables(list_axes(g, filter, w, h, dw, dh), t);
        set_tile_axes(in, t);
    }
    const RectListRoute route = route_yuv_rect_list(rects.data(), n, in);
    fill_plan(plan, route, yuv_list_desc_bytes(route));
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
    YuvRouteInputs ri = route_inputs(g, w, h, dw, dh, c.mode, foreign_capture(c));
    Tables t;
    if (may_batch(ri)) {
        if ((rc = get_tables(c, list_axes(g, filter, w, h, dw, dh), t))) return rc;
        set_tile_axes(ri, t);
    }
    const RectListRoute route = route_yuv_rect_list(rects.data(), n, ri);
    const Source s{g, in, w, h};
    const Shell sh{s, t, dsts.data()};
    if (!route.cells.empty() && (rc = list_batched(c, sh, dw, dh, route, rects.data()))) return rc;
    for (unsigned k : route.single) {
        const ListRect& r = rects[k];
        if ((rc = yuv_rect(c, g, w, h, dw, dh, filter, in, outs.data() + (size_t)3 * k, r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh))) return rc;
    }
    return SRCNN_OK;
}

}  // extern "C"
