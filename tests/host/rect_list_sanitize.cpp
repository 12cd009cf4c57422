// rect_list_sanitize.cpp -- CPU-only sanitizer harness for the host half of the rect list call (include/srcnn_amd_rect_list.h):
// no GPU, no HIP.  Built and run by tests/test_rect_list_sanitizer.py with -fsanitize=address,undefined, the way
// tests/test_yuv_rect_sanitizer.py builds its program.  What runs under the sanitizers is libsrcnn_amd/csrc/srcnn_rect_atlas.hpp:
// the router (rect_item_batched, route_rect_list), the shelf packer (pack_rect_cells) and the descriptor tables with their tile
// prefix sums (build_cell_descs), over seeded lists: n = 1, 65536 one-sample rects, one frame-sized rect among small ones
// (routed single by the threshold, and batched when the threshold is lifted), rects on every border, and workspace caps that
// force many atlases.  For every list it asserts that
//   * every item is placed exactly once: in `single`, or in one cell of one pass;
//   * every cell lies inside its atlas, and the atlas obeys the cap (a cell that is alone in its atlas excepted: the router has
//     checked it against the cap) and the Y path's limits;
//   * cells are pairwise disjoint (every atlas sample is painted at most once);
//   * the tile prefix sums of a pass start at 0, grow by exactly the tiles of each cell, and end in the closing entry;
//   * the in-plane part of a cell lies inside the cell and inside the plane, and the same list packs the same way twice;
//   * the staging buffer filled through ListTableLayout is the tables of the passes one after another, every byte of it belongs
//     to exactly one pass, and it has the bytes the plan call reports for the tables.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libsrcnn_amd/csrc/resample_table.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_rect_atlas.hpp"

using namespace srcnn;

static int g_fail = 0;
#define CHECK(cond, ...)                                                                  \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            ++g_fail;                                                                     \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond);                  \
            std::printf(__VA_ARGS__);                                                     \
            std::printf("\n");                                                            \
            if (g_fail > 20) { std::printf("too many failures\n"); std::exit(1); }        \
        }                                                                                 \
    } while (0)

struct Rng {      // splitmix64: the lists are the same on every machine
    unsigned long long s;
    unsigned long long next() { unsigned long long z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    unsigned below(unsigned n) { return (unsigned)(next() % n); }
};

struct Frame {
    unsigned w, h, dw, dh;
    AxisTable th, tv;
    Frame(unsigned w_, unsigned h_, unsigned dw_, unsigned dh_) : w(w_), h(h_), dw(dw_), dh(dh_), th(build_axis_table(2, dw_, w_)), tv(build_axis_table(2, dh_, h_)) {}
    RouteInputs inputs(unsigned long long cap, unsigned long long single) const
    {
        RouteInputs in;
        in.w = w; in.h = h; in.dw = dw; in.dh = dh;
        in.cap_bytes = cap; in.single_samples = single;
        in.th = TileAxis{th.first.data(), th.taps.data(), th.max_taps};
        in.tv = TileAxis{tv.first.data(), tv.taps.data(), tv.max_taps};
        return in;
    }
};

static ListRect random_rect(Rng& g, const Frame& f, unsigned max_side)
{
    ListRect r;
    r.rw = 1 + g.below(std::min(max_side, f.dw));
    r.rh = 1 + g.below(std::min(max_side, f.dh));
    r.x0 = g.below(f.dw - r.rw + 1);
    r.y0 = g.below(f.dh - r.rh + 1);
    switch (g.below(8)) {      // a few touch the borders
    case 0: r.x0 = 0; break;
    case 1: r.y0 = 0; break;
    case 2: r.x0 = f.dw - r.rw; break;
    case 3: r.y0 = f.dh - r.rh; break;
    default: break;
    }
    return r;
}

// The staging buffer as the batched route fills it (list_batched, srcnn_rect_list_call.hpp): every pass's table copied to where
// ListTableLayout puts it.  `all`: the tables of the passes one after another, as check_route has built and checked them.
static void check_layout(const char* what, const RectListRoute& route, const std::vector<ListRect>& rects, const std::vector<ListOut>& outs, const Frame& f,
                         const std::vector<ListCellDesc>& all)
{
    const ListTableLayout lay(route, 0, 0);        // the Y list: one table
    std::vector<unsigned char> buf(lay.bytes, 0xa5), writes(lay.bytes, 0);
    std::vector<ListCellDesc> d;
    for (size_t k = 0; k < route.passes.size(); ++k) {
        if (!build_cell_descs(route, route.passes[k], rects.data(), outs.data(), f.dw, f.dh, d)) return;      // (check_route has said so)
        const size_t at = lay.cell_first(route, k) * sizeof(ListCellDesc), n = d.size() * sizeof(ListCellDesc);
        CHECK(at + n <= lay.bytes, "%s: the table of pass %zu ends at byte %zu of %zu", what, k, at + n, lay.bytes);
        if (at + n > lay.bytes) return;
        std::copy(d.begin(), d.end(), lay.cells(buf.data(), route, k));
        for (size_t b = at; b < at + n; ++b) ++writes[b];
    }
    size_t holes = 0, twice = 0;
    for (unsigned char w : writes) { holes += w == 0; twice += w > 1; }
    CHECK(holes == 0 && twice == 0, "%s: %zu bytes of the staging buffer belong to no pass, %zu to two", what, holes, twice);
    CHECK(lay.bytes == all.size() * sizeof(ListCellDesc) && (lay.bytes == 0 || std::memcmp(buf.data(), all.data(), lay.bytes) == 0),
          "%s: the staging buffer (%zu bytes) is not the tables of the passes one after another (%zu entries)", what, lay.bytes, all.size());
    // what srcnn_y_path_rect_list_plan counts beside the atlas: a cell entry per batched item and the closing entry of every atlas
    CHECK(lay.dst_offset == lay.bytes && lay.bytes == (route.cells.size() + route.passes.size()) * sizeof(ListCellDesc), "%s: %zu bytes of tables for %zu cells in %zu passes",
          what, lay.bytes, route.cells.size(), route.passes.size());
}

static void check_route(const char* what, const Frame& f, const std::vector<ListRect>& rects, const RouteInputs& in, unsigned want_min_passes)
{
    const unsigned n = (unsigned)rects.size();
    const RectListRoute route = route_rect_list(rects.data(), n, in);
    const RectListRoute again = route_rect_list(rects.data(), n, in);
    std::vector<unsigned char> seen(n, 0);
    for (unsigned k : route.single) { CHECK(k < n, "%s: single %u", what, k); if (k < n) { CHECK(!seen[k], "%s: item %u twice", what, k); seen[k] = 1; } }
    CHECK(route.passes.size() >= want_min_passes, "%s: %zu passes, want at least %u", what, route.passes.size(), want_min_passes);
    CHECK(again.cells.size() == route.cells.size() && again.passes.size() == route.passes.size() && again.atlas_samples == route.atlas_samples,
          "%s: a second run packs differently", what);
    const unsigned long long cap = in.cap_bytes / kAtlasSampleBytes;
    unsigned long long cell_sum = 0, atlas_sum = 0;
    size_t next = 0;
    std::vector<ListOut> outs(n);
    for (unsigned k = 0; k < n; ++k) outs[k] = ListOut{reinterpret_cast<void*>((uintptr_t)0x1000 + 16u * k), rects[k].rw};
    std::vector<ListCellDesc> d, all;       // all: the tables of every pass, one after another
    for (size_t p = 0; p < route.passes.size(); ++p) {
        const AtlasPass& a = route.passes[p];
        CHECK(a.first == next && a.count > 0 && a.first + (size_t)a.count <= route.cells.size(), "%s: pass %zu covers [%u, +%u)", what, p, a.first, a.count);
        next = a.first + (size_t)a.count;
        CHECK(a.W > 0 && a.H > 0 && a.W <= kAtlasMaxW && a.H <= kAtlasMaxH, "%s: pass %zu is %ux%u", what, p, a.W, a.H);
        CHECK(a.count == 1 || (unsigned long long)a.W * a.H <= cap, "%s: pass %zu, %ux%u over the cap of %llu samples", what, p, a.W, a.H, cap);
        atlas_sum += (unsigned long long)a.W * a.H;
        std::vector<unsigned char> paint((size_t)a.W * a.H, 0);
        for (unsigned k = 0; k < a.count && a.first + (size_t)k < route.cells.size(); ++k) {
            const AtlasCell& c = route.cells[a.first + k];
            CHECK(again.cells[a.first + k].item == c.item && again.cells[a.first + k].ax == c.ax && again.cells[a.first + k].ay == c.ay, "%s: cell %u moved", what, k);
            CHECK(c.item < n && c.pass == p, "%s: cell of item %u in pass %u", what, c.item, c.pass);
            if (c.item >= n) continue;
            CHECK(!seen[c.item], "%s: item %u twice", what, c.item);
            seen[c.item] = 1;
            const ListRect& r = rects[c.item];
            CHECK(c.cw == r.rw + 12 && c.ch == r.rh + 12, "%s: cell of item %u is %ux%u", what, c.item, c.cw, c.ch);
            CHECK(rect_item_batched(r, in), "%s: item %u is batched against the rules", what, c.item);
            const bool inside = (unsigned long long)c.ax + c.cw <= a.W && (unsigned long long)c.ay + c.ch <= a.H;
            CHECK(inside, "%s: cell of item %u at (%u,%u) %ux%u leaves the %ux%u atlas", what, c.item, c.ax, c.ay, c.cw, c.ch, a.W, a.H);
            cell_sum += (unsigned long long)c.cw * c.ch;
            if (!inside) continue;
            bool clash = false;
            for (unsigned y = 0; y < c.ch; ++y) {
                unsigned char* row = &paint[(size_t)(c.ay + y) * a.W + c.ax];
                for (unsigned x = 0; x < c.cw; ++x) { clash = clash || row[x]; row[x] = 1; }
            }
            CHECK(!clash, "%s: the cell of item %u overlaps another", what, c.item);
        }
        // descriptors and prefix sums
        const bool ok = build_cell_descs(route, a, rects.data(), outs.data(), f.dw, f.dh, d);
        CHECK(ok && d.size() == (size_t)a.count + 1, "%s: descriptors of pass %zu", what, p);
        if (!ok) continue;
        unsigned long long rs = 0, rep = 0, sc = 0;
        for (unsigned k = 0; k < a.count; ++k) {
            const ListCellDesc& e = d[k];
            const ListRect& r = rects[route.cells[a.first + k].item];
            CHECK(e.rs_tile0 == rs && e.rep_tile0 == rep && e.sc_tile0 == sc, "%s: prefix sums of cell %u", what, k);
            CHECK(e.iw > 0 && e.ih > 0 && e.ox + e.iw <= e.cw && e.oy + e.ih <= e.ch, "%s: in-plane part of cell %u", what, k);
            CHECK((unsigned long long)e.px + e.iw <= f.dw && (unsigned long long)e.py + e.ih <= f.dh, "%s: cell %u leaves the plane", what, k);
            CHECK(e.px + 6 == r.x0 + e.ox && e.py + 6 == r.y0 + e.oy, "%s: cell %u is not anchored at its rect", what, k);
            CHECK(e.ox <= 6 && e.oy <= 6 && e.ox + e.iw >= 6 + r.rw && e.oy + e.ih >= 6 + r.rh, "%s: the rect of cell %u is not in-plane", what, k);
            CHECK(e.rw == r.rw && e.rh == r.rh && e.out_stride == r.rw, "%s: rect of cell %u", what, k);
            const bool border = e.iw != e.cw || e.ih != e.ch;
            CHECK(border == (r.x0 < 6 || r.y0 < 6 || r.x0 + r.rw + 6 > f.dw || r.y0 + r.rh + 6 > f.dh), "%s: border flag of cell %u", what, k);
            rs += (unsigned long long)((e.iw + 63) / 64) * ((e.ih + 15) / 16);
            rep += border ? (unsigned long long)((e.cw + 63) / 64) * ((e.ch + 15) / 16) : 0;
            sc += (unsigned long long)((e.rw + 63) / 64) * ((e.rh + 15) / 16);
        }
        CHECK(d[a.count].rs_tile0 == rs && d[a.count].rep_tile0 == rep && d[a.count].sc_tile0 == sc, "%s: closing entry of pass %zu", what, p);
        all.insert(all.end(), d.begin(), d.end());
    }
    check_layout(what, route, rects, outs, f, all);
    CHECK(next == route.cells.size(), "%s: %zu cells, passes cover %zu", what, route.cells.size(), next);
    for (unsigned k = 0; k < n; ++k) CHECK(seen[k], "%s: item %u is nowhere", what, k);
    CHECK(cell_sum == route.cell_samples && atlas_sum == route.atlas_samples, "%s: sums", what);
    std::printf("%-44s n %6u  batched %6zu  single %6zu  atlases %4zu  fill %.3f\n", what, n, route.cells.size(), route.single.size(), route.passes.size(),
                route.atlas_samples ? (double)route.cell_samples / (double)route.atlas_samples : 0.0);
}

int main()
{
    const unsigned long long GiB = 1ull << 30;
    const Frame small(96, 56, 192, 112), big(3840, 2160, 7680, 4320);
    Rng g{20240607};
    {
        std::vector<ListRect> one{{5, 7, 3, 2}};
        check_route("n = 1", small, one, small.inputs(4 * GiB, 2097152), 1);
        one[0] = ListRect{0, 0, 192, 112};
        check_route("n = 1, the whole frame", small, one, small.inputs(4 * GiB, 2097152), 1);
    }
    {
        std::vector<ListRect> v;
        for (unsigned k = 0; k < 64; ++k) v.push_back(random_rect(g, small, 40));
        check_route("64 rects of 1...40", small, v, small.inputs(4 * GiB, 2097152), 1);
        const RectListRoute r = route_rect_list(v.data(), 64, small.inputs(4 * GiB, 2097152));
        CHECK(r.single.empty() && r.atlas_samples <= 2 * r.cell_samples, "64 rects: %zu single, %llu atlas samples for %llu", r.single.size(), r.atlas_samples, r.cell_samples);
        check_route("64 rects of 1...40, cap 1 MiB", small, v, small.inputs(1 << 20, 2097152), 3);
        check_route("64 rects of 1...40, cap 128 KiB", small, v, small.inputs(128 << 10, 2097152), 4);
    }
    for (unsigned n : {16u, 17u, 23u, 24u, 25u, 26u, 37u, 50u, 65u, 101u, 256u}) {
        for (unsigned side : {1u, 32u, 100u}) {
            std::vector<ListRect> v;
            for (unsigned k = 0; k < n; ++k) { ListRect r = random_rect(g, big, 1); r.rw = r.rh = side; r.x0 = std::min(r.x0, big.dw - side); r.y0 = std::min(r.y0, big.dh - side); v.push_back(r); }
            char name[64];
            std::snprintf(name, sizeof name, "%u equal cells of %u", n, side + 12);
            check_route(name, big, v, big.inputs(4 * GiB, 2097152), 1);
            const RectListRoute r = route_rect_list(v.data(), n, big.inputs(4 * GiB, 2097152));
            CHECK(r.atlas_samples * 2 <= 3 * r.cell_samples, "%s: %llu atlas samples for %llu", name, r.atlas_samples, r.cell_samples);
        }
    }
    {
        std::vector<ListRect> v;
        for (unsigned k = 0; k < 65536; ++k) { ListRect r = random_rect(g, big, 1); v.push_back(r); }
        check_route("65536 one-sample rects", big, v, big.inputs(4 * GiB, 2097152), 1);
        check_route("65536 one-sample rects, cap 16 MiB", big, v, big.inputs(16 << 20, 2097152), 2);
    }
    {
        std::vector<ListRect> v;
        for (unsigned k = 0; k < 200; ++k) v.push_back(random_rect(g, big, 64));
        v.insert(v.begin() + 77, ListRect{0, 0, big.dw, big.dh});
        check_route("a frame-sized rect among small ones", big, v, big.inputs(5 * GiB, 2097152), 1);
        const RectListRoute r = route_rect_list(v.data(), (unsigned)v.size(), big.inputs(5 * GiB, 2097152));
        CHECK(r.single.size() == 1 && r.single[0] == 77, "the frame-sized rect is single (%zu single)", r.single.size());
        check_route("the same, threshold lifted", big, v, big.inputs(5 * GiB, ~0ull), 1);
        check_route("the same, threshold lifted, cap 1 GiB", big, v, big.inputs(1 * GiB, ~0ull), 1);
    }
    {
        std::vector<ListRect> v;      // tall and wide strips: the narrow-atlas fallback of the packer
        for (unsigned k = 0; k < 40; ++k) v.push_back(k & 1 ? ListRect{g.below(7000), 0, 1 + g.below(8), 4000} : ListRect{0, g.below(4000), 7000, 1 + g.below(8)});
        for (unsigned k = 0; k < 100; ++k) v.push_back(random_rect(g, big, 300));
        check_route("strips and blocks", big, v, big.inputs(5 * GiB, 2097152), 1);
        check_route("strips and blocks, cap 24 MiB", big, v, big.inputs(24 << 20, 2097152), 4);
        check_route("strips and blocks, cap 1 MiB", big, v, big.inputs(1 << 20, 2097152), 1);
    }
    {
        std::vector<ListRect> v;      // nothing may batch: a down-scale, an identity axis, unfused, a mode that is not strict
        for (unsigned k = 0; k < 32; ++k) v.push_back(ListRect{k % 20, k % 11, 1 + k % 9, 1 + k % 7});
        const Frame down(50, 30, 37, 20), ident(96, 56, 192, 56);
        RouteInputs in = down.inputs(4 * GiB, 2097152);
        CHECK(route_rect_list(v.data(), 32, in).cells.empty(), "a down-scale batches");
        in = ident.inputs(4 * GiB, 2097152);
        CHECK(route_rect_list(v.data(), 32, in).cells.empty(), "an identity axis batches");
        in = small.inputs(4 * GiB, 2097152); in.unfused = true;
        CHECK(route_rect_list(v.data(), 32, in).cells.empty(), "unfused batches");
        in = small.inputs(4 * GiB, 2097152); in.strict = false;
        CHECK(route_rect_list(v.data(), 32, in).cells.empty(), "a non-strict mode batches");
        in = small.inputs(4 * GiB, 2097152); in.th = TileAxis{nullptr, nullptr, 0};
        CHECK(route_rect_list(v.data(), 32, in).cells.empty(), "tables without host copies batch");
        check_route("all single", down, v, down.inputs(4 * GiB, 2097152), 0);
    }
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
