// yuv_packed_rect_list_sanitize.cpp -- CPU-only sanitizer harness for the host half of the packed YUV rect list call
// (include/srcnn_amd_yuv_packed_rect_list.h): no GPU, no HIP.  Built and run by tests/test_yuv_packed_rect_list_sanitizer.py with
// -fsanitize=address,undefined, the way tests/test_yuv_rect_list_sanitizer.py builds its program.  What runs under the sanitizers
// is libsrcnn_amd/csrc/srcnn_yuv_packed_rect_atlas.hpp on top of srcnn_rect_atlas.hpp: the router with the chroma condition
// (yuv_packed_rect_item_batched, route_yuv_packed_rect_list) and the destination table (build_yuv_packed_dst_descs), over seeded
// lists in all six kinds (YUY2, Y210, VUYA, Y410, Y416, v210) with destinations inside one arena per list: tight, pitched, and at
// bases of every alignment the format allows.  For every list it asserts that
//   * every destination entry belongs to exactly one batched item (entry k of a pass is the item of cell k of that pass), and
//     every batched item has one;
//   * chroma columns, rows, luma width and groups of the entry are the item's;
//   * the chroma tile prefix counts each item's tiles exactly once -- 64 x 16, 60 x 16 for v210 -- and its total is the closing
//     entry's;
//   * the bytes an entry lets k_yuvp_list_merge write -- recomputed from the descriptors alone, tile by tile and item by item as
//     yuvp_merge_tile walks them -- are exactly the item's rh row segments of n bytes at its pitch, v210's padding groups included
//     only where the rect reaches the right border;
//   * [blo, bhi) lies inside the span of the source rectangle the single call reports for the item;
//   * the vector store path is flagged only where base and pitch are multiples of 16 (and is flagged where they are);
//   * an item whose chroma window does not fit the tile resampler is routed single, whatever the Y list says about it;
//   * a frame whose chroma width keeps its size while luma grows routes every item single.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libsrcnn_amd/csrc/resample_table.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_yuv_packed_rect_atlas.hpp"

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

struct Frame {
    int format;
    YuvPackedGeom g;
    unsigned w, h, dw, dh;
    float mul;
    int filter;
    AxisTable th, tv, cth, ctv;
    Frame(int format_, unsigned w_, unsigned h_, float mul_, int filter_ = 2) : format(format_), w(w_), h(h_), dw(0), dh(0), mul(mul_), filter(filter_)
    {
        if (yuv_packed_geom(format, g) || srcnn_output_size(w, h, mul, 0, &dw, &dh)) { std::printf("bad frame\n"); std::exit(1); }
        const int cf = filter == 0 ? 0 : 1;
        th = build_axis_table(filter, dw, w);
        tv = build_axis_table(filter, dh, h);
        cth = build_axis_table(cf, g.ccols(dw), g.ccols(w));
        ctv = build_axis_table(cf, dh, h);
    }
    int kind() const { return g.rule.kind; }
    YuvPackedRouteInputs inputs(unsigned long long cap, unsigned long long single) const
    {
        YuvPackedRouteInputs in;
        in.kind = kind();
        in.y.w = w; in.y.h = h; in.y.dw = dw; in.y.dh = dh;
        in.y.cap_bytes = cap; in.y.single_samples = single;
        in.y.th = TileAxis{th.first.data(), th.taps.data(), th.max_taps};
        in.y.tv = TileAxis{tv.first.data(), tv.taps.data(), tv.max_taps};
        in.cth = TileAxis{cth.first.data(), cth.taps.data(), cth.max_taps};
        in.ctv = TileAxis{ctv.first.data(), ctv.taps.data(), ctv.max_taps};
        return in;
    }
};

// a rect under the format's unit rule: the origin snapped down, the far edge up to the unit or to dw
static ListRect random_rect(Rng& g, const Frame& f, unsigned max_side)
{
    const unsigned unit = yuv_packed_unit(f.kind());
    ListRect r;
    r.rw = 1 + g.below(std::min(max_side, f.dw));
    r.rh = 1 + g.below(std::min(max_side, f.dh));
    r.x0 = g.below(f.dw - r.rw + 1);
    r.y0 = g.below(f.dh - r.rh + 1);
    const unsigned x1 = std::min(f.dw, (r.x0 + r.rw + unit - 1) / unit * unit);
    r.x0 -= r.x0 % unit;
    r.rw = x1 - r.x0;
    return r;
}

// bytes of a row segment of the item, from the item alone
static size_t span_bytes(const Frame& f, const ListRect& r)
{
    size_t off = 0, n = 0;
    yuv_packed_span(f.kind(), f.dw, r.x0, r.rw, off, n);
    return n;
}

// Destinations of a list inside one arena (never dereferenced by the code under test; the painting below indexes a shadow of it)
struct Arena {
    std::vector<YuvPackedListDst> dst;
    size_t bytes = 0;
    uintptr_t base = 0x10000;       // the address the arena pretends to start at: 16-byte aligned, so offsets decide alignment
};

static Arena lay_out(Rng& g, const std::vector<ListRect>& rects, const Frame& f)
{
    Arena a;
    size_t pos = 0;
    const unsigned al = f.g.align;
    for (const ListRect& r : rects) {
        const size_t n = span_bytes(f, r);
        YuvPackedListDst q{};
        const unsigned how = g.below(4);
        // tight / 16-byte multiples / anything the format allows
        q.pitch = how == 0 ? n : how == 1 ? ((n + 15) & ~(size_t)15) + 16 * g.below(3) : n + al * g.below(9);
        pos = ((pos + 15) & ~(size_t)15) + (g.below(2) ? al * g.below(16 / al) : 0);       // aligned, or at any alignment the format allows
        q.dst = reinterpret_cast<void*>(a.base + pos);
        pos += q.pitch * (r.rh - 1) + n + 8;                                               // (a gap after every item)
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

// what an item of yuvp_merge_tile is (PkShape / PkItem of the kernels, restated without HIP)
struct Item { unsigned cpi, chunks, tile, ipr; };
static Item item_of(int kind)
{
    const bool v210 = kind == kPkV210;
    const unsigned nc = kind == kPk422x8 || kind == kPk444x8 || kind == kPk410 ? 4u : v210 ? 3u : 2u;      // chroma samples of a 16-byte chunk
    const unsigned cpi = v210 ? 3u : kTileChunk, tile = yuv_packed_tile_cols(kind);
    return Item{cpi, cpi / nc, tile, tile / cpi};
}

// What k_yuvp_list_merge stores for one entry: workgroups [ch_tile0, next.ch_tile0), each a tile of the entry's chroma grid
static void paint_merge(const YuvPackedListDstDesc& o, unsigned next_tile0, int kind, const Painter& P)
{
    const Item I = item_of(kind);
    const bool v210 = kind == kPkV210;
    const unsigned tiles_x = (o.ccols + I.tile - 1) / I.tile;
    for (unsigned b = o.ch_tile0; b < next_tile0; ++b) {
        const unsigned tile = b - o.ch_tile0, bx = tile % tiles_x, by = tile / tiles_x, tx = bx * I.tile, ty = by * kTileH;
        CHECK(tx < o.ccols && ty < o.rh, "%s: tile %u lies outside its %u x %u chroma grid", P.what, tile, o.ccols, o.rh);
        if (tx >= o.ccols || ty >= o.rh) continue;
        const unsigned ncol = std::min(I.tile, o.ccols - tx), nrow = std::min((unsigned)kTileH, o.rh - ty);
        unsigned ipr = I.ipr;
        if (v210 && bx == tiles_x - 1) {
            CHECK(o.groups >= bx * I.ipr, "%s: %u groups, the last tile starts at group %u", P.what, o.groups, bx * I.ipr);
            ipr = o.groups - bx * I.ipr;
        }
        for (unsigned ry = 0; ry < nrow; ++ry)
            for (unsigned i = 0; i < ipr; ++i) {
                const unsigned c = i * I.cpi, n = c < ncol ? std::min(I.cpi, ncol - c) : 0u;
                if (!v210 && n == 0) continue;
                const unsigned nd = v210 ? 4u : n * (4 * I.chunks / I.cpi);
                const unsigned long long d = o.dst + (unsigned long long)(ty + ry) * o.pitch + (unsigned long long)((tx + c) / I.cpi) * (16 * I.chunks);
                if (nd == 4 * I.chunks && o.io == (unsigned)kIoVec) {
                    for (unsigned j = 0; j < I.chunks; ++j) P.mark(d + 16 * j, 16, 16);
                } else {
                    const unsigned piece = o.io == (unsigned)kIoVec ? (unsigned)kIoDword : o.io;
                    for (unsigned j = 0; j < nd; ++j)
                        for (unsigned q = 0; q < 4; q += piece) P.mark(d + 4 * j + q, piece, piece);
                }
            }
    }
}

struct Tally { size_t vec = 0, pieces = 0, padded = 0, short_v210 = 0; };

static void check_list(const char* what, const Frame& fr, const std::vector<ListRect>& rects, const YuvPackedRouteInputs& in, Rng& g, bool expect_all_batched,
                       Tally& tally)
{
    const int kind = fr.kind();
    const unsigned n = (unsigned)rects.size();
    const Arena a = lay_out(g, rects, fr);
    const RectListRoute route = route_yuv_packed_rect_list(rects.data(), n, in);
    if (expect_all_batched) CHECK(route.single.empty(), "%s: %zu items single", what, route.single.size());
    std::vector<unsigned char> owner(n, 0), paint(a.bytes, 0), want(a.bytes, 0);
    std::vector<ListCellDesc> d;
    std::vector<YuvPackedListDstDesc> dd;
    const Painter P{a, paint, what};
    const unsigned tile = kind == kPkV210 ? 60u : 64u;
    size_t entries = 0;
    for (const AtlasPass& pass : route.passes) {
        const bool ok = build_cell_descs(route, pass, rects.data(), nullptr, fr.dw, fr.dh, d) &&
                        build_yuv_packed_dst_descs(route, pass, rects.data(), a.dst.data(), kind, fr.w, fr.dw, in.cth, dd);
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
            const YuvPackedListDst& q = a.dst[item];
            const YuvPackedListDstDesc& o = dd[k];
            const size_t nb = span_bytes(fr, r);
            CHECK(yuv_packed_rect_item_batched(r, in), "%s: item %u is batched against the rules", what, item);
            CHECK(d[k].rw == r.rw && d[k].rh == r.rh && d[k].px + kCellMargin - d[k].ox == r.x0 && d[k].py + kCellMargin - d[k].oy == r.y0,
                  "%s: cell %u does not give back the rect of item %u", what, k, item);
            const unsigned step = yuv_packed_chroma_step(kind), cx0 = r.x0 / step, cx1 = (r.x0 + r.rw + step - 1) / step;
            CHECK(o.cx0 == cx0 && o.ccols == cx1 - cx0 && o.y0 == r.y0 && o.rw == r.rw && o.rh == r.rh, "%s: chroma columns / rows of item %u", what, item);
            CHECK(o.groups == nb / 16, "%s: %u groups for %zu bytes of item %u", what, o.groups, nb, item);
            CHECK(o.dst == (unsigned long long)reinterpret_cast<uintptr_t>(q.dst) && o.pitch == q.pitch, "%s: destination of item %u", what, item);
            CHECK(o.ch_tile0 == tiles, "%s: entry %u starts at tile %u, %llu tiles lie ahead of it", what, k, o.ch_tile0, tiles);
            tiles += (unsigned long long)((cx1 - cx0 + tile - 1) / tile) * ((r.rh + 15) / 16);
            const bool vec = o.dst % 16 == 0 && o.pitch % 16 == 0;
            CHECK((o.io == (unsigned)kIoVec) == vec, "%s: store path %u of item %u, base %llu pitch %llu", what, o.io, item, o.dst, o.pitch);
            CHECK(o.io == (unsigned)kIoVec || (o.dst % o.io == 0 && o.pitch % o.io == 0 && (o.io == 4 || o.io == 2 || o.io == 1)), "%s: pieces of %u for item %u", what, o.io, item);
            (vec ? tally.vec : tally.pieces) += 1;
            if (kind == kPkV210) (r.x0 + r.rw == fr.dw && nb > (size_t)16 * ((r.rw + 5) / 6) ? tally.padded : tally.short_v210) += 1;
            // the source bytes the chroma taps may read lie inside the span of the source rectangle the single call reports
            unsigned sx0 = 0, sy0 = 0, sw = 0, sh = 0;
            const int rc = yuv_packed_rect_source(fr.format, fr.w, fr.h, fr.mul, fr.filter, r.x0, r.y0, r.rw, r.rh, &sx0, &sy0, &sw, &sh);
            CHECK(rc == 0, "%s: source rectangle of item %u: %d", what, item, rc);
            size_t soff = 0, sn = 0;
            yuv_packed_span(kind, fr.w, sx0, sw, soff, sn);
            CHECK(o.blo < o.bhi && o.blo >= soff && o.bhi <= soff + sn && o.blo % 4 == 0 && o.bhi % 4 == 0,
                  "%s: item %u may read bytes [%u, %u) of a row, its source rectangle spans [%zu, %zu)", what, item, o.blo, o.bhi, soff, soff + sn);
            paint_merge(o, dd[k + 1].ch_tile0, kind, P);
            // the item's own bytes, from the item alone
            for (unsigned y = 0; y < r.rh; ++y)
                for (size_t b = 0; b < nb; ++b) ++want[reinterpret_cast<uintptr_t>(q.dst) - a.base + y * q.pitch + b];
        }
        CHECK(dd[pass.count].ch_tile0 == tiles, "%s: the closing entry says %u tiles, the items have %llu", what, dd[pass.count].ch_tile0, tiles);
    }
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
    Rng g{20241020};
    char name[112];
    size_t lists = 0;
    Tally tally;
    static const struct { int format; const char* name; } kKinds[] = {{SRCNN_YUVP_YUY2, "YUY2"}, {SRCNN_YUVP_Y210, "Y210"}, {SRCNN_YUVP_VUYA, "VUYA"},
                                                                       {SRCNN_YUVP_Y410, "Y410"}, {SRCNN_YUVP_Y416, "Y416"}, {SRCNN_YUVP_V210, "v210"}};
    for (const auto& kd : kKinds) {
        const Frame small(kd.format, 96, 56, 2.0f), edge(kd.format, 70, 40, 2.0f), odd(kd.format, 35, 20, 2.5f), near(kd.format, 37, 21, 2.5f, 0);
        const unsigned unit = yuv_packed_unit(small.kind());
        std::vector<ListRect> v;
        for (unsigned k = 0; k < 64; ++k) v.push_back(random_rect(g, small, 40));
        v.push_back(ListRect{0, 0, small.dw, small.dh});
        v.push_back(ListRect{small.dw - unit, small.dh - 1, unit, 1});
        v.push_back(ListRect{6, 4, 132, 17});            // more than one tile of chroma columns for every kind
        v.push_back(ListRect{0, 0, 126, 33});
        std::snprintf(name, sizeof name, "%s: 2x", kd.name);
        check_list(name, small, v, small.inputs(4 * GiB, 2097152), g, true, tally);
        std::snprintf(name, sizeof name, "%s: 2x, cap 1 MiB", kd.name);
        check_list(name, small, v, small.inputs(1 << 20, 2097152), g, false, tally);
        for (const Frame* fr : {&edge, &odd}) {         // 140 is no multiple of 6 (padding groups), 87 is odd (the empty slot)
            v.clear();
            for (unsigned k = 0; k < 40; ++k) v.push_back(random_rect(g, *fr, 50));
            for (unsigned k = 1; k <= 8; ++k) v.push_back(ListRect{fr->dw - std::min(fr->dw, k * 12u) / unit * unit - fr->dw % unit, k, std::min(fr->dw, k * 12u) / unit * unit + fr->dw % unit, 3 * k});
            v.push_back(ListRect{0, 0, fr->dw, fr->dh});
            std::snprintf(name, sizeof name, "%s: %ux%u -> %ux%u", kd.name, fr->w, fr->h, fr->dw, fr->dh);
            check_list(name, *fr, v, fr->inputs(4 * GiB, 2097152), g, true, tally);
        }
        v.clear();
        for (unsigned k = 0; k < 40; ++k) v.push_back(random_rect(g, near, 52));
        std::snprintf(name, sizeof name, "%s: x2.5 nearest, threshold 1000", kd.name);
        check_list(name, near, v, near.inputs(4 * GiB, 1000), g, false, tally);
        lists += 5;
    }
    CHECK(lists == 30, "%zu lists", lists);
    CHECK(tally.vec && tally.pieces, "both store paths occur (%zu %zu)", tally.vec, tally.pieces);
    CHECK(tally.padded && tally.short_v210, "v210 rects with padding groups and without occur (%zu %zu)", tally.padded, tally.short_v210);
    {
        // the chroma condition: tables the tile resampler does not serve send an item the single way although its Y window fits
        const Frame small(SRCNN_YUVP_V210, 96, 56, 2.0f);
        std::vector<ListRect> v;
        for (unsigned k = 0; k < 32; ++k) v.push_back(random_rect(g, small, 40));
        YuvPackedRouteInputs in = small.inputs(4 * GiB, 2097152);
        CHECK(route_yuv_packed_rect_list(v.data(), 32, in).single.empty(), "the list batches with its own tables");
        in.cth = TileAxis{nullptr, nullptr, 0};
        CHECK(route_yuv_packed_rect_list(v.data(), 32, in).cells.empty() && route_rect_list(v.data(), 32, in.y).single.empty(), "chroma tables without host copies batch");
        // a vertical chroma table whose taps straddle more than the patch from output row 60 on (the frame has 56 rows, the patch
        // 24): rects with a tile that holds two such rows are single, the others batched
        in = small.inputs(4 * GiB, 2097152);
        std::vector<int> wide_first(small.ctv.first), wide_taps(small.ctv.taps);
        for (unsigned y = 60; y < small.dh; ++y) { wide_first[y] = (y & 1) ? 0 : (int)small.h - 2; wide_taps[y] = 2; }
        in.ctv = TileAxis{wide_first.data(), wide_taps.data(), small.ctv.max_taps};
        const RectListRoute route = route_yuv_packed_rect_list(v.data(), 32, in);
        size_t reach = 0;
        for (unsigned k : route.single) {
            CHECK(!yuvp_chroma_tile_way(v[k], in) && rect_item_batched(v[k], in.y), "item %u is single for another reason", k);
            CHECK(v[k].y0 + v[k].rh > 61, "item %u does not reach the doctored rows", k);
            ++reach;
        }
        for (const AtlasCell& c : route.cells) CHECK(yuvp_chroma_tile_way(v[c.item], in), "item %u is batched with a chroma window that does not fit", c.item);
        CHECK(reach > 0 && reach < 32, "the doctored table splits the list (%zu single)", reach);
        Tally t2;
        check_list("doctored chroma table", small, v, in, g, false, t2);
        // v210's tile is 60 chroma columns: a horizontal table whose columns [0, 60) read source columns [0, 2) and whose columns
        // [60, 96) read [80, 82) fits tiles of 60 and does not fit tiles of 64 -- the predicate must ask at 60, other kinds at 64
        in = small.inputs(4 * GiB, 2097152);
        CHECK(yuvp_window_fits(kPkV210, in.cth, in.ctv, 0, 96, 0, 16) && window_tile_fits(in.cth, in.ctv, 0, 96, 0, 16), "the real tables fit at 60 and at 64");
        std::vector<int> hf(small.cth.first), ht(small.cth.taps);
        for (unsigned x = 0; x < 96; ++x) { hf[x] = x < 60 ? 0 : 80; ht[x] = 2; }
        in.cth = TileAxis{hf.data(), ht.data(), small.cth.max_taps};
        CHECK(yuvp_window_fits(kPkV210, in.cth, in.ctv, 0, 96, 0, 16), "the v210 predicate asks tiles of 60");
        CHECK(!yuvp_window_fits(kPk422x16, in.cth, in.ctv, 0, 96, 0, 16) && !window_tile_fits(in.cth, in.ctv, 0, 96, 0, 16), "the other kinds ask tiles of 64");
        // a mode that is not strict, and the switch
        in = small.inputs(4 * GiB, 2097152); in.y.strict = false;
        CHECK(route_yuv_packed_rect_list(v.data(), 32, in).cells.empty(), "a non-strict mode batches");
        in = small.inputs(4 * GiB, 2097152); in.y.unfused = true;
        CHECK(route_yuv_packed_rect_list(v.data(), 32, in).cells.empty(), "unfused batches");
    }
    {
        // a chroma width that keeps its size while luma grows: every item is single, although the Y list would batch every one
        for (int format : {SRCNN_YUVP_YUY2, SRCNN_YUVP_Y210, SRCNN_YUVP_V210}) {
            const Frame fr(format, 1, 9, 2.0f);
            CHECK(fr.dw == 2 && fr.dh == 18 && fr.g.ccols(fr.dw) == fr.g.ccols(fr.w), "1 -> 2 keeps its chroma column");
            std::vector<ListRect> v;
            for (unsigned k = 0; k < 16; ++k) v.push_back(random_rect(g, fr, 20));
            v.push_back(ListRect{0, 0, fr.dw, fr.dh});
            const YuvPackedRouteInputs in = fr.inputs(4 * GiB, 2097152);
            const RectListRoute route = route_yuv_packed_rect_list(v.data(), (unsigned)v.size(), in);
            CHECK(route.cells.empty() && route.passes.empty() && route.single.size() == v.size(), "format %d, 1x9 -> 2x18: %zu items batched", format, route.cells.size());
            CHECK(route_rect_list(v.data(), (unsigned)v.size(), in.y).single.empty(), "format %d, 1x9 -> 2x18: the Y list batches every item", format);
        }
        // 4:4:4 has no such axis: the same frame batches
        const Frame fr444(SRCNN_YUVP_Y410, 1, 9, 2.0f);
        std::vector<ListRect> v;
        for (unsigned k = 0; k < 16; ++k) v.push_back(random_rect(g, fr444, 20));
        CHECK(route_yuv_packed_rect_list(v.data(), (unsigned)v.size(), fr444.inputs(4 * GiB, 2097152)).single.empty(), "1x9 -> 2x18 in 4:4:4 batches");
    }
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
