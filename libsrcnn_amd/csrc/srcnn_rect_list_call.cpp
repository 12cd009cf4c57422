// srcnn_rect_list_call.cpp -- the rect LIST call (include/srcnn_amd_rect_list.h): its argument checks, and what the Y plane adds
// to the list skeleton (srcnn_rect_list_call.hpp: routing, the descriptor upload and the launches of an atlas): the resample
// and the scatter of srcnn_rect_list.hip.  Single items go through y_path_rect of srcnn_capi.cpp, exactly as the single call
// runs it.
#include <vector>

#include "../../include/srcnn_amd_rect.h"
#include "../../include/srcnn_amd_rect_list.h"
#include "srcnn_frame_args.hpp"
#include "srcnn_rect_list_call.hpp"

using namespace srcnn;

// ---- a list of rectangles of the output (include/srcnn_amd_rect_list.h) ---------------------------
namespace {

static_assert(sizeof(ListCellDesc) == 80, "the header states 80 B per batched item");

// What both list entry points refuse before they look at an item.  SRCNN_OK with n == 0: nothing to do.
int check_rect_list_frame(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const srcnn_rect_item* items, unsigned n, unsigned item_size)
{
    if (const int rc = check_list_header(items, n, item_size, sizeof(srcnn_rect_item), "srcnn_rect_item")) return rc;
    if (n == 0) return SRCNN_OK;
    if (w == 0 || h == 0) return fail(SRCNN_E_ARG, "zero dimension (%ux%u)", w, h);
    if (dw == 0 || dh == 0) return fail(SRCNN_E_SCALE, "scaled size %ux%u", dw, dh);
    if (filter < 0 || filter > 4) return fail(SRCNN_E_ARG, "bad filter %d", filter);
    return SRCNN_OK;
}

RouteInputs route_inputs(unsigned w, unsigned h, unsigned dw, unsigned dh, int mode, bool foreign)
{
    return list_route_inputs(w, h, dw, dh, mode, foreign || settings().rect_list_unfused);
}

// The Y plane in the skeleton: no destination table (the cell table carries d_out), the plane's own resample, the scatter.
struct Shell {
    using Dst = NoDst;
    static constexpr unsigned kDstClosing = 0;
    static constexpr const char* kTrace = "srcnn rect list";
    static constexpr const char* kName = "y_path_rect_list";
    const float* d_in;
    size_t in_stride;
    unsigned w, h;
    const TableRef &th, &tv;
    const ListOut* out;
    const ListOut* outs() const { return out; }
    bool build_dst(const RectListRoute&, const AtlasPass&, const ListRect*, std::vector<NoDst>&) const { return true; }
    void fill(Call& c, const ListPass<NoDst>& p) const
    {
        launch_list_resample(d_in, in_stride, w, h, th->view(), tv->view(), p.d, p.count, p.end, c.ws->up.data(), p.W, c.s);
    }
    void store(Call& c, const ListPass<NoDst>& p) const { launch_list_scatter(p.d, p.count, p.end, c.ws->win.data(), p.W, c.s); }
};

}  // namespace

extern "C" {

int srcnn_rect_list_abi_version(void) { return SRCNN_AMD_RECT_LIST_VERSION; }

int srcnn_y_path_rect_list_plan(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const srcnn_rect_item* items, unsigned n,
                                unsigned item_size, srcnn_rect_list_plan* plan)
{
    int rc;
    if ((rc = check_plan(plan))) return rc;
    if ((rc = check_rect_list_frame(w, h, dw, dh, filter, items, n, item_size))) return rc;
    if (n == 0) { fill_plan(plan, RectListRoute{}, 0); return SRCNN_OK; }
    std::vector<ListRect> rects(n);
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_rect_item& it = items[k];
        if ((rc = check_rect_geometry(w, h, dw, dh, filter, it.x0, it.y0, it.rw, it.rh))) return fail_item(rc, k);
        if ((rc = check_rect_limits(w, h, dw, dh, it.rh))) return fail_item(rc, k);
        rects[k] = ListRect{it.x0, it.y0, it.rw, it.rh};
    }
    RouteInputs in = route_inputs(w, h, dw, dh, G.mode.load(), false);
    AxisTable th, tv;
    if (list_may_batch(in)) {
        th = build_axis_table(filter, dw, w);
        tv = build_axis_table(filter, dh, h);
        in.th = tile_axis(th);
        in.tv = tile_axis(tv);
    }
    const RectListRoute route = route_rect_list(rects.data(), n, in);
    fill_plan(plan, route, ListTableLayout(route, 0, 0).bytes);
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
    RouteInputs ri = route_inputs(w, h, dw, dh, c.mode, foreign_capture(c));
    TableRef th, tv;
    if (list_may_batch(ri)) {
        if ((rc = get_table(c, filter, dw, w, th))) return rc;
        if ((rc = get_table(c, filter, dh, h, tv))) return rc;
        ri.th = tile_axis(th);
        ri.tv = tile_axis(tv);
    }
    const RectListRoute route = route_rect_list(rects.data(), n, ri);
    const size_t in_stride = in.pitch / sizeof(float);
    const Shell sh{d_in, in_stride, w, h, th, tv, outs.data()};
    if (!route.cells.empty() && (rc = list_batched(c, sh, dw, dh, route, rects.data()))) return rc;
    for (unsigned k : route.single) {
        const ListRect& r = rects[k];
        if ((rc = y_path_rect(c, d_in, in_stride, 0, 0, w, h, dw, dh, filter, r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh, static_cast<float*>(outs[k].d_out), outs[k].out_stride)))
            return rc;
    }
    return SRCNN_OK;
}

}  // extern "C"
