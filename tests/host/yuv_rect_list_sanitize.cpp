// yuv_rect_list_sanitize.cpp -- CPU-only sanitizer harness for the host half of the planar / semi-planar YUV rect list call
// (include/srcnn_amd_yuv_rect_list.h): no GPU, no HIP.  Built and run by tests/test_yuv_rect_list_sanitizer.py with
// -fsanitize=address,undefined, the way tests/test_rgb_rect_list_sanitizer.py builds its program.  What runs under the sanitizers
// is libsrcnn_amd/csrc/srcnn_yuv_rect_atlas.hpp on top of srcnn_rect_atlas.hpp: the router with the chroma condition
// (yuv_rect_item_batched, route_yuv_rect_list) and the destination table (build_yuv_dst_descs), over seeded lists in every cell
// -- 4:2:0 / 4:2:2 / 4:4:4, planar and semi-planar, 1 / 2 bytes per sample -- with destinations inside one arena per list: tight,
// pitched, and at bases of every alignment the format allows.  For every list it asserts that
//   * every destination entry belongs to exactly one batched item (entry k of a pass is the item of cell k of that pass), and
//     every batched item has one;
//   * the chroma rect in the entry is YuvChromaRect of the item;
//   * the chroma tile prefix counts each item's 64 x 16 tiles exactly once, and its total is the closing entry's;
//   * the bytes an entry lets k_yuv_list_luma and k_yuv_list_chroma write -- recomputed from the descriptors alone, tile by tile
//     as the kernels walk them -- are exactly the item's rows at its pitches, plane by plane;
//   * a vector flag is set only where every base and pitch it covers is a multiple of the store size (and is set where they are);
//   * an item whose chroma window does not fit the tile resampler is routed single, whatever the Y list says about it;
//   * a frame whose chroma axis keeps its size while luma grows routes every item single;
//   * the staging buffer filled through ListTableLayout (srcnn_rect_atlas.hpp) is the cell tables of the passes and then their
//     destination tables, closing entries included, every byte of it belongs to exactly one table, and it has the bytes the plan
//     call reports for the tables.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libsrcnn_amd/csrc/resample_table.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_yuv_rect_atlas.hpp"

// The product's fail() lives in srcnn_capi.cpp; this one formats as well, so the sanitizers see every message's arguments.
namespace srcnn {
int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace srcnn

// (csrc/dropin.cpp's, for stepscale == 0: the only form the frame calls use)
extern "C" int srcnn_output_size(unsigned w, unsigned h, float multiply, int stepscale, unsigned* out_w, unsigned* out_h)
{
    if (w == 0 || h == 0) return -1;
    if ((float)w * multiply <= 0.f || (float)h * multiply <= 0.f || stepscale) return -2;
    const unsigned cw = (unsigned)((float)w * multiply), ch = (unsigned)((float)h * multiply);
    if (cw == 0 || ch == 0) return -2;
    *out_w = cw; *out_h = ch;
    return 0;
}

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

static YuvGeom geom(bool semi, unsigned sx, unsigned sy, unsigned bps)
{
    YuvGeom g;
    g.semi = semi; g.sx = sx; g.sy = sy; g.bps = bps;
    return g;
}

struct Frame {
    YuvGeom g;
    unsigned w, h, dw, dh;
    AxisTable th, tv, cth, ctv;
    Frame(const YuvGeom& g_, unsigned w_, unsigned h_, unsigned dw_, unsigned dh_, int filter = 2)
        : g(g_), w(w_), h(h_), dw(dw_), dh(dh_), th(build_axis_table(filter, dw_, w_)), tv(build_axis_table(filter, dh_, h_)),
          cth(build_axis_table(filter == 0 ? 0 : 1, g_.ccols(dw_), g_.ccols(w_))), ctv(build_axis_table(filter == 0 ? 0 : 1, g_.crows(dh_), g_.crows(h_))) {}
    YuvRouteInputs inputs(unsigned long long cap, unsigned long long single) const
    {
        YuvRouteInputs in;
        in.g = g;
        in.y.w = w; in.y.h = h; in.y.dw = dw; in.y.dh = dh;
        in.y.cap_bytes = cap; in.y.single_samples = single;
        in.y.th = TileAxis{th.first.data(), th.taps.data(), th.max_taps};
        in.y.tv = TileAxis{tv.first.data(), tv.taps.data(), tv.max_taps};
        in.cth = TileAxis{cth.first.data(), cth.taps.data(), cth.max_taps};
        in.ctv = TileAxis{ctv.first.data(), ctv.taps.data(), ctv.max_taps};
        return in;
    }
};

// a rect under the format's origin rule
static ListRect random_rect(Rng& g, const Frame& f, unsigned max_side)
{
    ListRect r;
    r.rw = 1 + g.below(std::min(max_side, f.dw));
    r.rh = 1 + g.below(std::min(max_side, f.dh));
    r.x0 = g.below(f.dw - r.rw + 1);
    r.y0 = g.below(f.dh - r.rh + 1);
    if (f.g.sx && (r.x0 & 1)) { --r.x0; ++r.rw; }
    if (f.g.sy && (r.y0 & 1)) { --r.y0; ++r.rh; }
    return r;
}

// columns, rows and row bytes of plane p (0: luma, 1 / 2: chroma) of the item's destination, from the item alone
struct PlaneShape { unsigned rows; size_t row_bytes; };
static PlaneShape plane_shape(const YuvGeom& g, const ListRect& r, unsigned p)
{
    if (p == 0) return PlaneShape{r.rh, (size_t)g.bps * r.rw};
    const YuvChromaRect cr(g, r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh);
    return PlaneShape{cr.cy1 - cr.cy0, (size_t)g.bps * (g.semi ? 2u : 1u) * (cr.cx1 - cr.cx0)};
}

// Destinations of a list inside one arena (never dereferenced by the code under test; the painting below indexes a shadow of it)
struct Arena {
    std::vector<YuvListDst> dst;
    size_t bytes = 0;
    uintptr_t base = 0x10000;       // the address the arena pretends to start at: 16-byte aligned, so offsets decide alignment
};

static Arena lay_out(Rng& g, const std::vector<ListRect>& rects, const YuvGeom& f)
{
    Arena a;
    size_t pos = 0;
    const unsigned np = f.semi ? 2u : 3u;
    for (const ListRect& r : rects) {
        YuvListDst q{};
        for (unsigned p = 0; p < np; ++p) {
            const PlaneShape s = plane_shape(f, r, p);
            const unsigned how = g.below(4);
            // tight / 16-byte multiples / anything the format allows
            q.pitch[p] = how == 0 ? s.row_bytes : how == 1 ? ((s.row_bytes + 15) & ~(size_t)15) + 16 * g.below(3) : s.row_bytes + f.bps * g.below(9);
            pos = ((pos + 15) & ~(size_t)15) + (g.below(2) ? f.bps * g.below(8) : 0);        // aligned, or at any alignment the format allows
            q.plane[p] = reinterpret_cast<void*>(a.base + pos);
            pos += q.pitch[p] * (s.rows - 1) + s.row_bytes + 8;                             // (a gap after every plane)
        }
        a.dst.push_back(q);
    }
    a.bytes = pos + 32;
    return a;
}

struct Painter {
    const Arena& a;
    std::vector<unsigned char>& paint;
    const char* what;
    void mark(unsigned long long addr, size_t n, unsigned align) const
    {
        CHECK(addr % align == 0, "%s: a %u-byte store at an address that is %llu mod %u", what, align, addr % align, align);
        CHECK(addr >= a.base && addr - a.base + n <= a.bytes, "%s: a store leaves the arena", what);
        if (addr < a.base || addr - a.base + n > a.bytes) return;
        for (size_t k = 0; k < n; ++k) ++paint[(size_t)(addr - a.base) + k];
    }
};

// What k_yuv_list_luma stores for one cell, off the two descriptors alone: tiles of 64 x 16 of the rect, 4 samples per thread, as
// one store where the flag allows it and the 4 samples are whole.
static void paint_luma(const ListCellDesc& c, const YuvListDstDesc& o, const YuvGeom& f, const Painter& P)
{
    const unsigned tiles_x = (c.rw + kTileW - 1) / kTileW, tiles = tiles_of(c.rw, c.rh);
    for (unsigned tile = 0; tile < tiles; ++tile)
        for (unsigned t = 0; t < (unsigned)kTileThreads; ++t) {
            const unsigned y = (tile / tiles_x) * kTileH + t / (kTileW / kTileChunk), x = (tile % tiles_x) * kTileW + (t % (kTileW / kTileChunk)) * kTileChunk;
            if (y >= c.rh || x >= c.rw) continue;
            const unsigned nn = std::min(kTileChunk, c.rw - x);
            const unsigned long long q = o.plane[0] + (size_t)y * o.pitch[0] + (size_t)x * f.bps;
            if (nn == kTileChunk && o.luma_vec) P.mark(q, (size_t)kTileChunk * f.bps, yuv_luma_store_bytes(f));
            else P.mark(q, (size_t)nn * f.bps, f.bps);
        }
}

// What k_yuv_list_chroma stores for one entry: workgroups [ch_tile0, next.ch_tile0), each a 64 x 16 tile of the entry's chroma rect
static void paint_chroma(const YuvListDstDesc& o, unsigned next_tile0, const YuvGeom& f, const Painter& P)
{
    const unsigned spp = f.semi ? 2u : 1u, tiles_x = (o.ccols + kTileW - 1) / kTileW;
    for (unsigned b = o.ch_tile0; b < next_tile0; ++b) {
        const unsigned tile = b - o.ch_tile0, tx = (tile % tiles_x) * kTileW, ty = (tile / tiles_x) * kTileH;
        CHECK(tx < o.ccols && ty < o.crows, "%s: chroma tile %u lies outside its %u x %u rect", P.what, tile, o.ccols, o.crows);
        if (tx >= o.ccols || ty >= o.crows) continue;
        const unsigned ncol = std::min((unsigned)kTileW, o.ccols - tx), nrow = std::min((unsigned)kTileH, o.crows - ty);
        for (unsigned ry = 0; ry < nrow; ++ry)
            for (unsigned cc = 0; cc < ncol; cc += kTileChunk) {
                const unsigned n = std::min(kTileChunk, ncol - cc);
                const size_t dr = (size_t)ty + ry, dc = (size_t)tx + cc;
                for (unsigned p = 1; p <= (f.semi ? 1u : 2u); ++p) {
                    const unsigned long long q = o.plane[p] + dr * o.pitch[p] + dc * spp * f.bps;
                    if (n == kTileChunk && o.chroma_vec) P.mark(q, (size_t)kTileChunk * spp * f.bps, yuv_chroma_store_bytes(f));
                    else P.mark(q, (size_t)n * spp * f.bps, f.bps);
                }
            }
    }
}

struct Tally { size_t lvec = 0, lscalar = 0, cvec = 0, cscalar = 0; };

// The staging buffer as the batched route fills it (list_batched, srcnn_rect_list_call.hpp): both tables of every pass copied to
// where ListTableLayout puts them -- two tables, each with a closing entry per pass.  all_cells / all_dst: the tables of the
// passes one after another, as check_list has built and checked them.
static void check_layout(const char* what, const Frame& fr, const RectListRoute& route, const std::vector<ListRect>& rects, const Arena& a,
                         const std::vector<ListCellDesc>& all_cells, const std::vector<YuvListDstDesc>& all_dst)
{
    const ListTableLayout lay(route, sizeof(YuvListDstDesc), 1);
    std::vector<unsigned char> buf(lay.bytes, 0xa5), writes(lay.bytes, 0);
    std::vector<ListCellDesc> d;
    std::vector<YuvListDstDesc> dd;
    for (size_t k = 0; k < route.passes.size(); ++k) {
        const AtlasPass& pass = route.passes[k];
        if (!build_cell_descs(route, pass, rects.data(), nullptr, fr.dw, fr.dh, d) || !build_yuv_dst_descs(route, pass, rects.data(), a.dst.data(), fr.g, dd))
            return;                                                                                  // (check_list has said so)
        const size_t at = lay.cell_first(route, k) * sizeof(ListCellDesc), n = d.size() * sizeof(ListCellDesc);
        const size_t at_dst = lay.dst_offset + lay.dst_first(route, k) * sizeof(YuvListDstDesc), n_dst = dd.size() * sizeof(YuvListDstDesc);
        CHECK(at + n <= lay.dst_offset && at_dst + n_dst <= lay.bytes, "%s: the tables of pass %zu end at bytes %zu of %zu and %zu of %zu", what, k, at + n,
              lay.dst_offset, at_dst + n_dst, lay.bytes);
        if (at + n > lay.dst_offset || at_dst + n_dst > lay.bytes) return;
        std::copy(d.begin(), d.end(), lay.cells(buf.data(), route, k));
        std::copy(dd.begin(), dd.end(), lay.dsts<YuvListDstDesc>(buf.data(), route, k));
        for (size_t b = at; b < at + n; ++b) ++writes[b];
        for (size_t b = at_dst; b < at_dst + n_dst; ++b) ++writes[b];
    }
    size_t holes = 0, twice = 0;
    for (unsigned char w : writes) { holes += w == 0; twice += w > 1; }
    CHECK(holes == 0 && twice == 0, "%s: %zu bytes of the staging buffer belong to no table, %zu to two", what, holes, twice);
    const size_t cell_bytes = all_cells.size() * sizeof(ListCellDesc), dst_bytes = all_dst.size() * sizeof(YuvListDstDesc);
    CHECK(lay.dst_offset == cell_bytes && lay.bytes == cell_bytes + dst_bytes, "%s: %zu + %zu bytes of tables, the layout has %zu + %zu", what, cell_bytes, dst_bytes,
          lay.dst_offset, lay.bytes - lay.dst_offset);
    if (lay.dst_offset == cell_bytes && lay.bytes == cell_bytes + dst_bytes && lay.bytes)
        CHECK(std::memcmp(buf.data(), all_cells.data(), cell_bytes) == 0 && std::memcmp(buf.data() + cell_bytes, all_dst.data(), dst_bytes) == 0,
              "%s: the staging buffer is not the cell tables of the passes and then their destination tables", what);
    // what srcnn_yuv_upscale_rect_list_plan counts beside the atlas
    CHECK(lay.bytes == yuv_list_desc_bytes(route), "%s: the layout has %zu bytes, the plan reports %llu", what, lay.bytes, yuv_list_desc_bytes(route));
}

static void check_list(const char* what, const Frame& fr, const std::vector<ListRect>& rects, const YuvRouteInputs& in, Rng& g, bool expect_all_batched,
                       Tally& tally)
{
    const YuvGeom& f = fr.g;
    const unsigned n = (unsigned)rects.size(), np = f.semi ? 2u : 3u;
    const Arena a = lay_out(g, rects, f);
    const RectListRoute route = route_yuv_rect_list(rects.data(), n, in);
    if (expect_all_batched) CHECK(route.single.empty(), "%s: %zu items single", what, route.single.size());
    std::vector<unsigned char> owner(n, 0), paint(a.bytes, 0), want(a.bytes, 0);
    std::vector<ListCellDesc> d, all_cells;          // all_*: the tables of every pass, one after another
    std::vector<YuvListDstDesc> dd, all_dst;
    const Painter P{a, paint, what};
    size_t entries = 0;
    for (const AtlasPass& pass : route.passes) {
        const bool ok = build_cell_descs(route, pass, rects.data(), nullptr, fr.dw, fr.dh, d) && build_yuv_dst_descs(route, pass, rects.data(), a.dst.data(), f, dd);
        CHECK(ok && d.size() == (size_t)pass.count + 1 && dd.size() == (size_t)pass.count + 1, "%s: tables of a pass of %u cells", what, pass.count);
        if (!ok || dd.size() != (size_t)pass.count + 1) continue;
        entries += pass.count;
        unsigned long long tiles = 0;
        for (unsigned k = 0; k < pass.count; ++k) {
            const unsigned item = route.cells[pass.first + k].item;
            CHECK(item < n, "%s: cell of item %u", what, item);
            if (item >= n) continue;
            CHECK(!owner[item], "%s: item %u has two destination entries", what, item);
            owner[item] = 1;
            const ListRect& r = rects[item];
            const YuvListDst& q = a.dst[item];
            const YuvListDstDesc& o = dd[k];
            CHECK(yuv_rect_item_batched(r, in), "%s: item %u is batched against the rules", what, item);
            CHECK(d[k].rw == r.rw && d[k].rh == r.rh && d[k].px + kCellMargin - d[k].ox == r.x0 && d[k].py + kCellMargin - d[k].oy == r.y0,
                  "%s: cell %u does not give back the rect of item %u", what, k, item);
            const YuvChromaRect cr(f, r.x0, r.y0, r.x0 + r.rw, r.y0 + r.rh);
            CHECK(o.cx0 == cr.cx0 && o.cy0 == cr.cy0 && o.ccols == cr.cx1 - cr.cx0 && o.crows == cr.cy1 - cr.cy0, "%s: chroma rect of item %u", what, item);
            CHECK(o.ch_tile0 == tiles, "%s: entry %u starts at chroma tile %u, %llu tiles lie ahead of it", what, k, o.ch_tile0, tiles);
            tiles += tiles_of(cr.cx1 - cr.cx0, cr.cy1 - cr.cy0);
            const unsigned lb = 4 * f.bps, cb = 4 * f.bps * (f.semi ? 2 : 1);
            bool call = true;
            for (unsigned p = 0; p < 3; ++p) {
                if (p < np) {
                    CHECK(o.plane[p] == (unsigned long long)reinterpret_cast<uintptr_t>(q.plane[p]) && o.pitch[p] == q.pitch[p], "%s: plane %u of item %u", what, p, item);
                    if (p) call = call && o.plane[p] % cb == 0 && o.pitch[p] % cb == 0;
                } else {
                    CHECK(o.plane[p] == 0 && o.pitch[p] == 0, "%s: unused plane %u of item %u is set", what, p, item);
                }
            }
            const bool lall = o.plane[0] % lb == 0 && o.pitch[0] % lb == 0;
            CHECK(o.luma_vec == (lall ? 1u : 0u), "%s: luma flag %u of item %u, base %llu pitch %llu, store %u", what, o.luma_vec, item, o.plane[0], o.pitch[0], lb);
            CHECK(o.chroma_vec == (call ? 1u : 0u), "%s: chroma flag %u of item %u, store %u", what, o.chroma_vec, item, cb);
            (o.luma_vec ? tally.lvec : tally.lscalar) += 1;
            (o.chroma_vec ? tally.cvec : tally.cscalar) += 1;
            paint_luma(d[k], o, f, P);
            paint_chroma(o, dd[k + 1].ch_tile0, f, P);
            // the item's own bytes, from the item alone
            for (unsigned p = 0; p < np; ++p) {
                const PlaneShape s = plane_shape(f, r, p);
                for (unsigned y = 0; y < s.rows; ++y)
                    for (size_t b = 0; b < s.row_bytes; ++b) ++want[reinterpret_cast<uintptr_t>(q.plane[p]) - a.base + y * q.pitch[p] + b];
            }
        }
        CHECK(dd[pass.count].ch_tile0 == tiles, "%s: the closing entry says %u chroma tiles, the items have %llu", what, dd[pass.count].ch_tile0, tiles);
        all_cells.insert(all_cells.end(), d.begin(), d.end());
        all_dst.insert(all_dst.end(), dd.begin(), dd.end());
    }
    check_layout(what, fr, route, rects, a, all_cells, all_dst);
    CHECK(entries == route.cells.size(), "%s: %zu destination entries for %zu cells", what, entries, route.cells.size());
    for (unsigned k : route.single) { CHECK(k < n && !owner[k], "%s: single item %u has a destination entry", what, k); if (k < n) owner[k] = 2; }
    for (unsigned k = 0; k < n; ++k) CHECK(owner[k], "%s: item %u is nowhere", what, k);
    size_t wrong = 0, first = 0;
    for (size_t b = 0; b < a.bytes; ++b)
        if (paint[b] != want[b]) { if (!wrong) first = b; ++wrong; }
    CHECK(wrong == 0, "%s: %zu bytes are written that are not the item's, or the other way round; first at %zu (%u against %u)", what, wrong, first,
          (unsigned)paint[first], (unsigned)want[first]);
    std::printf("%-56s n %5u  batched %5zu  single %5zu  atlases %3zu\n", what, n, route.cells.size(), route.single.size(), route.passes.size());
}

int main()
{
    const unsigned long long GiB = 1ull << 30;
    Rng g{20240917};
    char name[112];
    size_t lists = 0;
    Tally tally;
    static const char* const kChroma[] = {"4:4:4", "4:2:2", "4:2:0"};
    for (unsigned sub = 0; sub < 3; ++sub)
        for (bool semi : {false, true})
            for (unsigned bps : {1u, 2u}) {
                const YuvGeom f = geom(semi, sub >= 1, sub >= 2, bps);
                const Frame small(f, 96, 56, 192, 112), odd(f, 40, 31, 60, 46), near(f, 37, 21, 92, 52, 0);
                std::vector<ListRect> v;
                for (unsigned k = 0; k < 64; ++k) v.push_back(random_rect(g, small, 40));
                v.push_back(ListRect{0, 0, small.dw, small.dh});
                v.push_back(ListRect{small.dw - 1 - (f.sx ? 1u : 0u), small.dh - 1 - (f.sy ? 1u : 0u), 1 + (f.sx ? 1u : 0u), 1 + (f.sy ? 1u : 0u)});
                v.push_back(ListRect{6, 4, 129, 17});
                v.push_back(ListRect{0, 0, 131, 33});          // a chroma rect of more than one tile where chroma is not subsampled
                std::snprintf(name, sizeof name, "%s, %s, %u B: 2x", kChroma[sub], semi ? "semi-planar" : "planar", bps);
                check_list(name, small, v, small.inputs(4 * GiB, 2097152), g, true, tally);
                std::snprintf(name, sizeof name, "%s, %s, %u B: 2x, cap 1 MiB", kChroma[sub], semi ? "semi-planar" : "planar", bps);
                check_list(name, small, v, small.inputs(1 << 20, 2097152), g, false, tally);
                v.clear();
                for (unsigned k = 0; k < 40; ++k) v.push_back(random_rect(g, odd, 46));
                std::snprintf(name, sizeof name, "%s, %s, %u B: x1.5", kChroma[sub], semi ? "semi-planar" : "planar", bps);
                check_list(name, odd, v, odd.inputs(4 * GiB, 2097152), g, true, tally);
                v.clear();
                for (unsigned k = 0; k < 40; ++k) v.push_back(random_rect(g, near, 52));
                std::snprintf(name, sizeof name, "%s, %s, %u B: x2.5 nearest, threshold 1000", kChroma[sub], semi ? "semi-planar" : "planar", bps);
                check_list(name, near, v, near.inputs(4 * GiB, 1000), g, false, tally);
                lists += 4;
            }
    CHECK(lists == 48, "%zu lists", lists);
    CHECK(tally.lvec && tally.lscalar && tally.cvec && tally.cscalar, "both store paths of both kernels occur (%zu %zu %zu %zu)", tally.lvec, tally.lscalar,
          tally.cvec, tally.cscalar);
    {
        // the chroma condition: tables the tile resampler does not serve send an item the single way although its Y window fits
        const YuvGeom f = geom(true, 1, 1, 1);      // NV12
        const Frame small(f, 96, 56, 192, 112);
        std::vector<ListRect> v;
        for (unsigned k = 0; k < 32; ++k) v.push_back(random_rect(g, small, 40));
        YuvRouteInputs in = small.inputs(4 * GiB, 2097152);
        CHECK(route_yuv_rect_list(v.data(), 32, in).single.empty(), "the list batches with its own tables");
        in.cth = TileAxis{nullptr, nullptr, 0};
        CHECK(route_yuv_rect_list(v.data(), 32, in).cells.empty() && route_rect_list(v.data(), 32, in.y).single.empty(), "chroma tables without host copies batch");
        // a vertical chroma table whose taps straddle more than the patch from chroma row 30 on (the chroma plane has 28 rows, the
        // patch 24): rects with a tile that holds two such rows are single, the others batched
        in = small.inputs(4 * GiB, 2097152);
        std::vector<int> wide_first(small.ctv.first), wide_taps(small.ctv.taps);
        const unsigned ch = f.crows(small.h), dch = f.crows(small.dh);
        for (unsigned y = 30; y < dch; ++y) { wide_first[y] = (y & 1) ? 0 : (int)ch - 2; wide_taps[y] = 2; }
        in.ctv = TileAxis{wide_first.data(), wide_taps.data(), small.ctv.max_taps};
        const RectListRoute route = route_yuv_rect_list(v.data(), 32, in);
        size_t reach = 0;
        for (unsigned k : route.single) {
            CHECK(!yuv_chroma_tile_way(v[k], in) && rect_item_batched(v[k], in.y), "item %u is single for another reason", k);
            const YuvChromaRect cr(f, v[k].x0, v[k].y0, v[k].x0 + v[k].rw, v[k].y0 + v[k].rh);
            CHECK(cr.cy1 > 31, "item %u does not reach the doctored rows", k);
            ++reach;
        }
        for (const AtlasCell& c : route.cells) CHECK(yuv_chroma_tile_way(v[c.item], in), "item %u is batched with a chroma window that does not fit", c.item);
        CHECK(reach > 0 && reach < 32, "the doctored table splits the list (%zu single)", reach);
        Tally t2;
        check_list("doctored chroma table", small, v, in, g, false, t2);
        // a mode that is not strict, and the switch
        in = small.inputs(4 * GiB, 2097152); in.y.strict = false;
        CHECK(route_yuv_rect_list(v.data(), 32, in).cells.empty(), "a non-strict mode batches");
        in = small.inputs(4 * GiB, 2097152); in.y.unfused = true;
        CHECK(route_yuv_rect_list(v.data(), 32, in).cells.empty(), "unfused batches");
    }
    {
        // a chroma axis that keeps its size while luma grows: every item is single, although the Y list would batch every one
        struct Kept { unsigned w, h, dw, dh; } kept[] = {{1, 9, 2, 18}, {3, 30, 4, 40}};      // 1 x 9 at 2x; w = 3 at 4/3: cw = dcw = 2
        for (const Kept& q : kept)
            for (bool semi : {false, true}) {
                const YuvGeom f = geom(semi, 1, 1, 1);
                const Frame fr(f, q.w, q.h, q.dw, q.dh);
                CHECK(f.ccols(q.dw) == f.ccols(q.w) && q.dw > q.w && q.dh > q.h, "%u -> %u keeps its chroma columns", q.w, q.dw);
                std::vector<ListRect> v;
                for (unsigned k = 0; k < 16; ++k) v.push_back(random_rect(g, fr, 20));
                v.push_back(ListRect{0, 0, q.dw, q.dh});
                const YuvRouteInputs in = fr.inputs(4 * GiB, 2097152);
                const RectListRoute route = route_yuv_rect_list(v.data(), (unsigned)v.size(), in);
                CHECK(route.cells.empty() && route.passes.empty() && route.single.size() == v.size(), "%ux%u -> %ux%u: %zu items batched", q.w, q.h, q.dw, q.dh,
                      route.cells.size());
                CHECK(route_rect_list(v.data(), (unsigned)v.size(), in.y).single.empty(), "%ux%u -> %ux%u: the Y list batches every item", q.w, q.h, q.dw, q.dh);
                // 4:4:4 has no such axis: the same frame batches
                const YuvGeom f444 = geom(semi, 0, 0, 1);
                const Frame fr444(f444, q.w, q.h, q.dw, q.dh);
                CHECK(route_yuv_rect_list(v.data(), (unsigned)v.size(), fr444.inputs(4 * GiB, 2097152)).single.empty(), "%ux%u -> %ux%u in 4:4:4 batches", q.w, q.h,
                      q.dw, q.dh);
            }
    }
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
