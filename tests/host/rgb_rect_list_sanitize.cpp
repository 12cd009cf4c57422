// rgb_rect_list_sanitize.cpp -- CPU-only sanitizer harness for the host half of the RGB(A) rect list call
// (include/srcnn_amd_rgb_rect_list.h): no GPU, no HIP.  Built and run by tests/test_rgb_rect_list_sanitizer.py with
// -fsanitize=address,undefined, the way tests/test_rect_list_sanitizer.py builds its program.  What runs under the sanitizers is
// libsrcnn_amd/csrc/srcnn_rgb_rect_atlas.hpp on top of srcnn_rect_atlas.hpp: the router with the chroma condition
// (rgb_rect_item_batched, route_rgb_rect_list) and the destination table (build_dst_descs), over seeded lists in every format
// cell -- 3 / 4 channels, 1 / 2 bytes per sample, planar and interleaved -- with destinations inside one arena per list: tight,
// pitched, and at bases of every alignment the format allows.  For every list it asserts that
//   * every destination entry belongs to exactly one batched item (entry k of a pass is the item of cell k of that pass), and
//     every batched item has one;
//   * the bytes an entry lets k_rgb_list_merge write -- recomputed from the two descriptors alone, tile by tile as the kernel
//     walks them -- are exactly the item's rh rows of rw pixels at its pitches, plane by plane and for dst_conv, and nothing of a
//     conv plane where the item has none;
//   * a vector flag is set only where every base and pitch it covers is a multiple of 4;
//   * an item whose chroma window does not fit the tile resampler is routed single, whatever the Y list says about it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libsrcnn_amd/csrc/resample_table.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_rgb_rect_atlas.hpp"

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
    AxisTable th, tv, cth, ctv;
    Frame(unsigned w_, unsigned h_, unsigned dw_, unsigned dh_, int filter = 2)
        : w(w_), h(h_), dw(dw_), dh(dh_), th(build_axis_table(filter, dw_, w_)), tv(build_axis_table(filter, dh_, h_)),
          cth(build_axis_table(filter == 0 ? 0 : 1, dw_, w_)), ctv(build_axis_table(filter == 0 ? 0 : 1, dh_, h_)) {}
    RgbRouteInputs inputs(unsigned long long cap, unsigned long long single) const
    {
        RgbRouteInputs in;
        in.y.w = w; in.y.h = h; in.y.dw = dw; in.y.dh = dh;
        in.y.cap_bytes = cap; in.y.single_samples = single;
        in.y.th = TileAxis{th.first.data(), th.taps.data(), th.max_taps};
        in.y.tv = TileAxis{tv.first.data(), tv.taps.data(), tv.max_taps};
        in.cth = TileAxis{cth.first.data(), cth.taps.data(), cth.max_taps};
        in.ctv = TileAxis{ctv.first.data(), ctv.taps.data(), ctv.max_taps};
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
    return r;
}

// Destinations of a list inside one arena (never dereferenced by the code under test; the painting below indexes a shadow of it)
struct Arena {
    std::vector<RgbListDst> dst;
    size_t bytes = 0;
    uintptr_t base = 0x10000;       // the address the arena pretends to start at: 4-byte aligned, so offsets decide alignment
};

static Arena lay_out(Rng& g, const std::vector<ListRect>& rects, const RgbListLayout& f)
{
    Arena a;
    size_t pos = 0;
    auto place = [&](size_t row, unsigned rh, void*& p, size_t& pitch) {
        const unsigned how = g.below(4);
        pitch = how == 0 ? row : how == 1 ? ((row + 3) & ~(size_t)3) + 4 * g.below(3) : row + f.bps * g.below(7);     // tight / 4-byte multiples / anything the format allows
        pos = ((pos + 3) & ~(size_t)3) + (g.below(2) ? f.bps * g.below(4) : 0);                                     // aligned, or at any alignment the format allows
        p = reinterpret_cast<void*>(a.base + pos);
        pos += pitch * (rh - 1) + row + 8;                                                                           // (a gap after every plane)
    };
    for (const ListRect& r : rects) {
        RgbListDst q{};
        for (unsigned p = 0; p < f.planes(); ++p) place(f.row_bytes(r.rw), r.rh, q.plane[p], q.pitch[p]);
        if (g.below(2)) place((size_t)f.bps * r.rw, r.rh, q.conv, q.conv_pitch);
        a.dst.push_back(q);
    }
    a.bytes = pos + 16;
    return a;
}

// What k_rgb_list_merge stores for one cell, off the two descriptors alone: tiles of 64 x 16, 4 pixels per thread, in 4-byte words
// where the flag allows it and the 4 pixels are whole.  paint: one counter per arena byte.
static void paint_cell(const ListCellDesc& c, const ListDstDesc& o, const RgbListLayout& f, const Arena& a, std::vector<unsigned char>& paint,
                       const char* what)
{
    const unsigned tiles_x = (c.rw + kTileW - 1) / kTileW, tiles = tiles_of(c.rw, c.rh);
    const size_t spp = f.planar ? 1 : f.ch;
    auto mark = [&](unsigned long long addr, size_t n, unsigned align) {
        CHECK(addr % align == 0, "%s: a %u-byte store at an address that is %llu mod %u", what, align, addr % align, align);
        CHECK(addr >= a.base && addr - a.base + n <= a.bytes, "%s: a store leaves the arena", what);
        if (addr < a.base || addr - a.base + n > a.bytes) return;
        for (size_t k = 0; k < n; ++k) ++paint[(size_t)(addr - a.base) + k];
    };
    for (unsigned tile = 0; tile < tiles; ++tile) {
        const unsigned tx = (tile % tiles_x) * kTileW, ty = (tile / tiles_x) * kTileH;
        const unsigned ncol = std::min((unsigned)kTileW, c.rw - tx), nrow = std::min((unsigned)kTileH, c.rh - ty);
        for (unsigned ry = 0; ry < nrow; ++ry)
            for (unsigned cc = 0; cc < ncol; cc += kTileChunk) {
                const unsigned n = std::min(kTileChunk, ncol - cc);
                const size_t dr = (size_t)ty + ry, dc = (size_t)tx + cc;
                for (unsigned p = 0; p < f.planes(); ++p) {
                    const unsigned long long q = o.plane[p] + dr * o.pitch[p] + dc * spp * f.bps;
                    if (n == kTileChunk && o.int_vec) mark(q, kTileChunk * spp * f.bps, 4);
                    else mark(q, n * spp * f.bps, f.bps);
                }
                if (o.conv) {
                    const unsigned long long q = o.conv + dr * o.conv_pitch + dc * f.bps;
                    if (n == kTileChunk && o.conv_vec) mark(q, (size_t)kTileChunk * f.bps, 4);
                    else mark(q, (size_t)n * f.bps, f.bps);
                }
            }
    }
}

static void check_list(const char* what, const Frame& fr, const std::vector<ListRect>& rects, const RgbListLayout& f, const RgbRouteInputs& in, Rng& g,
                       bool expect_all_batched)
{
    const unsigned n = (unsigned)rects.size();
    const Arena a = lay_out(g, rects, f);
    const RectListRoute route = route_rgb_rect_list(rects.data(), n, in);
    if (expect_all_batched) CHECK(route.single.empty(), "%s: %zu items single", what, route.single.size());
    std::vector<unsigned char> owner(n, 0), paint(a.bytes, 0), want(a.bytes, 0);
    std::vector<ListCellDesc> d;
    std::vector<ListDstDesc> dd;
    size_t entries = 0, vec = 0, scalar = 0;
    for (const AtlasPass& pass : route.passes) {
        const bool ok = build_cell_descs(route, pass, rects.data(), nullptr, fr.dw, fr.dh, d);
        build_dst_descs(route, pass, a.dst.data(), f, dd);
        CHECK(ok && d.size() == (size_t)pass.count + 1 && dd.size() == (size_t)pass.count, "%s: tables of a pass of %u cells", what, pass.count);
        if (!ok || dd.size() != pass.count) continue;
        entries += dd.size();
        for (unsigned k = 0; k < pass.count; ++k) {
            const unsigned item = route.cells[pass.first + k].item;
            CHECK(item < n, "%s: cell of item %u", what, item);
            if (item >= n) continue;
            CHECK(!owner[item], "%s: item %u has two destination entries", what, item);
            owner[item] = 1;
            const ListRect& r = rects[item];
            const RgbListDst& q = a.dst[item];
            const ListDstDesc& o = dd[k];
            CHECK(rgb_rect_item_batched(r, in), "%s: item %u is batched against the rules", what, item);
            CHECK(d[k].rw == r.rw && d[k].rh == r.rh && d[k].px + kCellMargin - d[k].ox == r.x0 && d[k].py + kCellMargin - d[k].oy == r.y0,
                  "%s: cell %u does not give back the rect of item %u", what, k, item);
            bool all4 = true;
            for (unsigned p = 0; p < 4; ++p) {
                if (p < f.planes()) {
                    CHECK(o.plane[p] == (unsigned long long)reinterpret_cast<uintptr_t>(q.plane[p]) && o.pitch[p] == q.pitch[p], "%s: plane %u of item %u", what, p, item);
                    all4 = all4 && o.plane[p] % 4 == 0 && o.pitch[p] % 4 == 0;
                } else {
                    CHECK(o.plane[p] == 0 && o.pitch[p] == 0, "%s: unused plane %u of item %u is set", what, p, item);
                }
            }
            CHECK(!o.int_vec || all4, "%s: item %u stores words through a base or pitch that is no multiple of 4", what, item);
            CHECK(o.int_vec == (all4 ? 1u : 0u), "%s: item %u misses the vector path it may take", what, item);
            CHECK(o.conv == (unsigned long long)reinterpret_cast<uintptr_t>(q.conv) && (!q.conv || o.conv_pitch == q.conv_pitch), "%s: conv of item %u", what, item);
            CHECK(!o.conv_vec || (o.conv && o.conv % 4 == 0 && o.conv_pitch % 4 == 0), "%s: conv flag of item %u", what, item);
            CHECK(q.conv || (!o.conv && !o.conv_vec), "%s: item %u has no conv plane, its entry has", what, item);
            (o.int_vec ? vec : scalar) += 1;
            paint_cell(d[k], o, f, a, paint, what);
            // the item's own bytes, from the item alone
            for (unsigned p = 0; p < f.planes(); ++p)
                for (unsigned y = 0; y < r.rh; ++y)
                    for (size_t b = 0; b < f.row_bytes(r.rw); ++b) ++want[reinterpret_cast<uintptr_t>(q.plane[p]) - a.base + y * q.pitch[p] + b];
            if (q.conv)
                for (unsigned y = 0; y < r.rh; ++y)
                    for (size_t b = 0; b < (size_t)f.bps * r.rw; ++b) ++want[reinterpret_cast<uintptr_t>(q.conv) - a.base + y * q.conv_pitch + b];
        }
    }
    CHECK(entries == route.cells.size(), "%s: %zu destination entries for %zu cells", what, entries, route.cells.size());
    for (unsigned k : route.single) { CHECK(k < n && !owner[k], "%s: single item %u has a destination entry", what, k); if (k < n) owner[k] = 2; }
    for (unsigned k = 0; k < n; ++k) CHECK(owner[k], "%s: item %u is nowhere", what, k);
    size_t wrong = 0, first = 0;
    for (size_t b = 0; b < a.bytes; ++b)
        if (paint[b] != want[b]) { if (!wrong) first = b; ++wrong; }
    CHECK(wrong == 0, "%s: %zu bytes are written that are not the item's, or the other way round; first at %zu (%u against %u)", what, wrong, first,
          (unsigned)paint[first], (unsigned)want[first]);
    std::printf("%-52s n %5u  batched %5zu  single %5zu  atlases %3zu  vector %5zu  scalar %5zu\n", what, n, route.cells.size(), route.single.size(),
                route.passes.size(), vec, scalar);
}

int main()
{
    const unsigned long long GiB = 1ull << 30;
    const Frame small(96, 56, 192, 112), odd(40, 31, 60, 46), near(37, 21, 92, 52, 0);
    Rng g{20240611};
    char name[96];
    size_t lists = 0;
    for (unsigned ch : {3u, 4u})
        for (unsigned bps : {1u, 2u})
            for (bool planar : {false, true}) {
                const RgbListLayout f{bps, ch, planar};
                std::vector<ListRect> v;
                for (unsigned k = 0; k < 64; ++k) v.push_back(random_rect(g, small, 40));
                v.push_back(ListRect{0, 0, small.dw, small.dh});
                v.push_back(ListRect{small.dw - 1, small.dh - 1, 1, 1});
                v.push_back(ListRect{7, 3, 129, 17});
                std::snprintf(name, sizeof name, "%u ch, %u B, %s: 2x", ch, bps, planar ? "planar" : "interleaved");
                check_list(name, small, v, f, small.inputs(4 * GiB, 2097152), g, true);
                std::snprintf(name, sizeof name, "%u ch, %u B, %s: 2x, cap 1 MiB", ch, bps, planar ? "planar" : "interleaved");
                check_list(name, small, v, f, small.inputs(1 << 20, 2097152), g, false);
                v.clear();
                for (unsigned k = 0; k < 40; ++k) v.push_back(random_rect(g, odd, 46));
                std::snprintf(name, sizeof name, "%u ch, %u B, %s: x1.5", ch, bps, planar ? "planar" : "interleaved");
                check_list(name, odd, v, f, odd.inputs(4 * GiB, 2097152), g, true);
                v.clear();
                for (unsigned k = 0; k < 40; ++k) v.push_back(random_rect(g, near, 52));
                std::snprintf(name, sizeof name, "%u ch, %u B, %s: x2.5 nearest, threshold 1000", ch, bps, planar ? "planar" : "interleaved");
                check_list(name, near, v, f, near.inputs(4 * GiB, 1000), g, false);
                lists += 4;
            }
    {
        // the chroma condition: tables the tile resampler does not serve send an item the single way although its Y window fits
        const RgbListLayout f{1, 3, false};
        std::vector<ListRect> v;
        for (unsigned k = 0; k < 32; ++k) v.push_back(random_rect(g, small, 40));
        RgbRouteInputs in = small.inputs(4 * GiB, 2097152);
        CHECK(route_rgb_rect_list(v.data(), 32, in).single.empty(), "the list batches with its own tables");
        in.cth = TileAxis{nullptr, nullptr, 0};
        CHECK(route_rgb_rect_list(v.data(), 32, in).cells.empty() && route_rect_list(v.data(), 32, in.y).single.empty(), "chroma tables without host copies batch");
        // a chroma table whose taps straddle more than the patch from column 100 on: rects that reach it are single, the others batched
        in = small.inputs(4 * GiB, 2097152);
        std::vector<int> wide_first(small.cth.first), wide_taps(small.cth.taps);
        for (unsigned x = 100; x < small.dw; ++x) { wide_first[x] = (x & 1) ? 0 : (int)small.w - 2; wide_taps[x] = 2; }
        in.cth = TileAxis{wide_first.data(), wide_taps.data(), small.cth.max_taps};
        const RectListRoute route = route_rgb_rect_list(v.data(), 32, in);
        size_t reach = 0;
        for (unsigned k : route.single) {
            CHECK(!window_tile_fits(in.cth, in.ctv, v[k].x0, v[k].rw, v[k].y0, v[k].rh) && rect_item_batched(v[k], in.y), "item %u is single for another reason", k);
            ++reach;
        }
        for (const AtlasCell& c : route.cells) CHECK(window_tile_fits(in.cth, in.ctv, v[c.item].x0, v[c.item].rw, v[c.item].y0, v[c.item].rh), "item %u is batched with a chroma window that does not fit", c.item);
        CHECK(reach > 0 && reach < 32, "the doctored table splits the list (%zu single)", reach);
        check_list("doctored chroma table", small, v, f, in, g, false);
        // a mode that is not strict, and the switch
        in = small.inputs(4 * GiB, 2097152); in.y.strict = false;
        CHECK(route_rgb_rect_list(v.data(), 32, in).cells.empty(), "a non-strict mode batches");
        in = small.inputs(4 * GiB, 2097152); in.y.unfused = true;
        CHECK(route_rgb_rect_list(v.data(), 32, in).cells.empty(), "unfused batches");
    }
    CHECK(lists == 32, "%zu lists", lists);
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
