// srcnn_delta_call.cpp -- the delta call (include/srcnn_amd_delta.h): its argument checks and the Y plane as a surface of the
// skeleton in srcnn_delta_call.hpp -- the Y path's span tables, the launch of k_delta_flags (srcnn_delta.hip) and the repaint.
// Nothing of the list call, the rect call or their kernels is changed: the rects go through the public
// srcnn_y_path_rect_list_f32_dev.
#include <vector>

#include "../../include/srcnn_amd_delta.h"
#include "srcnn_delta.h"
#include "srcnn_delta_call.hpp"
#include "srcnn_frame_args.hpp"

using namespace srcnn;

namespace {

// two float planes over one grid, and the output plane of the whole operation
struct YSurface {
    static constexpr DeltaSpanOwner kOwner = DeltaSpanOwner::YPlane;
    static constexpr const char *kTrace = "delta", *kName = "y_path_delta", *kEntry = "srcnn_y_path_delta_f32_dev";
    unsigned w, h, dw, dh;
    int filter;
    DeltaGrid grid;
    const float *d_prev, *d_cur;
    size_t cur_pitch;                                // as the caller gave it
    YuvPlane prev, cur, out;
    float* d_out = nullptr;

    bool has_prev() const { return d_prev != nullptr; }
    int spans(Call& c, std::vector<DeltaSpan>& xs, std::vector<DeltaSpan>& ys) const
    {
        int rc;
        TableRef th, tv;
        if (dw != w && (rc = get_table(c, filter, dw, w, th))) return rc;
        if (dh != h && (rc = get_table(c, filter, dh, h, tv))) return rc;
        delta_axis_spans(th ? th->h_first.data() : nullptr, th ? th->h_taps.data() : nullptr, dw, w, grid.tile_w, xs);
        delta_axis_spans(tv ? tv->h_first.data() : nullptr, tv ? tv->h_taps.data() : nullptr, dh, h, grid.tile_h, ys);
        return SRCNN_OK;
    }
    int queue_flags(Call& c, unsigned char* d_flags) const
    {
        launch_delta_flags(d_prev, prev.pitch, d_cur, cur.pitch, w, h, c.ws->delta_spans.data(), grid.cols, grid.rows, d_flags, c.s);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail(SRCNN_E_HIP, "y_path_delta_flags: %s", hipGetErrorString(e));
        return SRCNN_OK;
    }
    int repaint(const std::vector<DeltaRect>& rects, void* stream) const
    {
        std::vector<srcnn_rect_item> items(rects.size());
        delta_items(rects, d_out, out.pitch, items.data(), items.size());
        return srcnn_y_path_rect_list_f32_dev(d_cur, cur_pitch, w, h, dw, dh, filter, items.data(), (unsigned)items.size(), (unsigned)sizeof(srcnn_rect_item), stream);
    }
};

// the source planes and the grid: what both device entry points refuse before any device lookup
int check_delta_sources(const float* d_prev, size_t prev_pitch, const float* d_cur, size_t cur_pitch, unsigned w, unsigned h, unsigned dw,
                        unsigned dh, int filter, unsigned tile_w, unsigned tile_h, YSurface& a)
{
    int rc;
    if (!d_cur) return fail(SRCNN_E_ARG, "NULL d_cur");
    if ((rc = delta_grid(w, h, dw, dh, filter, tile_w, tile_h, a.grid))) return rc;
    a.w = w; a.h = h; a.dw = dw; a.dh = dh; a.filter = filter;
    a.d_prev = d_prev; a.d_cur = d_cur; a.cur_pitch = cur_pitch;
    if (d_prev && (rc = describe_plane(a.prev, d_prev, prev_pitch, sizeof(float) * (size_t)w, h, 4, "previous", 0))) return rc;
    return describe_plane(a.cur, d_cur, cur_pitch, sizeof(float) * (size_t)w, h, 4, "current", 0);
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
    YSurface a;
    if (!d_flags) return fail(SRCNN_E_ARG, "NULL d_flags");
    if (const int rc = check_delta_sources(d_prev, prev_pitch, d_cur, cur_pitch, w, h, dw, dh, filter, tile_w, tile_h, a)) return rc;
    return delta_flags_call(a, d_flags, stream);
}

int srcnn_y_path_delta_rects(const unsigned char* flags, unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h, unsigned dw,
                             unsigned dh, float* d_out, size_t out_pitch, srcnn_rect_item* items, unsigned cap, unsigned* n)
{
    if (!n) return fail(SRCNN_E_ARG, "NULL n");
    *n = 0;
    if (const int rc = check_delta_tiles(cols, rows, tile_w, tile_h, dw, dh)) return rc;
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
    YSurface a;
    if (!d_out) return fail(SRCNN_E_ARG, "NULL d_out");
    if ((rc = check_delta_stats(stats))) return rc;
    if ((rc = check_delta_sources(d_prev, prev_pitch, d_cur, cur_pitch, w, h, dw, dh, filter, tile_w, tile_h, a))) return rc;
    if ((rc = describe_plane(a.out, d_out, out_pitch, sizeof(float) * (size_t)dw, dh, 4, "output", 0))) return rc;
    if (d_prev && overlaps(a.prev, a.out)) return fail(SRCNN_E_ARG, "d_out overlaps d_prev");
    if (overlaps(a.cur, a.out)) return fail(SRCNN_E_ARG, "d_out overlaps d_cur");
    a.d_out = d_out;
    return delta_call(a, stream, stats);
}

}  // extern "C"
