// rgb_delta_sanitize.cpp -- CPU-only sanitizer harness for the host half of the RGB(A) delta call (include/srcnn_amd_rgb_delta.h):
// no GPU, no HIP.  Built and run by tests/test_rgb_delta_sanitizer.py with -fsanitize=address,undefined, the way
// tests/test_delta_sanitizer.py builds its program.  What runs under the sanitizers is libsrcnn_amd/csrc/srcnn_rgb_delta.hpp (the
// span tables of an RGB(A) grid, rgb_delta_axis_spans, and the items, rgb_delta_items) over the grid, the coalescer and the gate
// of srcnn_delta.hpp.  It asserts that
//   * the span of every tile column and row, built from ONE pair of tables per axis, is the union srcnn_rgb_rect_source computes
//     for that tile on its own -- y_path_rect_source_span united with axis_source_span of the chroma filter over the tile -- for
//     all five filters at 2x, 2.5x, 1.5x, the identity size, one axis that keeps its size and a down-scale, and that both ends
//     are monotone;
//   * the tiles the kernel's bisection finds for a source pixel are exactly the tiles whose span holds it;
//   * rgb_delta_items points every item at pixel (x0, y0) of the full-size image for every bytes-per-pixel class (3, 4, 6, 8
//     interleaved; 1, 2 planar), dst_conv likewise, writes nothing when the capacity is one short, and gives NULL destinations
//     for a NULL image.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libsrcnn_amd/csrc/srcnn_rgb_delta.hpp"

using namespace srcnn;

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
extern "C" int srcnn_output_size(unsigned, unsigned, float, int, unsigned*, unsigned*) { return SRCNN_E_ARG; }      // (check_scale is not used here)

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

// #{k < n : t[k] <= x}: the kernel's bisection
static unsigned count_le(const unsigned* t, unsigned n, unsigned x)
{
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (t[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

static unsigned g_chroma_wider = 0, g_luma_wider = 0;      // tiles where one part of the union reaches past the other

static void check_spans(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h)
{
    DeltaGrid g;
    CHECK(delta_grid(w, h, dw, dh, filter, tile_w, tile_h, g) == SRCNN_OK, "%ux%u -> %ux%u", w, h, dw, dh);
    std::vector<DeltaSpan> xs, ys;
    rgb_delta_axis_spans(filter, dw, w, g.tile_w, xs);
    rgb_delta_axis_spans(filter, dh, h, g.tile_h, ys);
    CHECK(xs.size() == g.cols && ys.size() == g.rows, "table sizes");
    CHECK(delta_spans_monotone(xs, w) && delta_spans_monotone(ys, h), "%ux%u -> %ux%u filter %d tile %ux%u", w, h, dw, dh, filter, g.tile_w, g.tile_h);
    const int cfilter = chroma_filter(filter);
    for (unsigned r = 0; r < g.rows; ++r)
        for (unsigned c = 0; c < g.cols; ++c) {
            const unsigned x0 = c * g.tile_w, y0 = r * g.tile_h, x1 = std::min(dw, x0 + g.tile_w), y1 = std::min(dh, y0 + g.tile_h);
            unsigned lx, hx, ly, hy, clx, chx, cly, chy;       // what srcnn_rgb_rect_source does for this rect
            y_path_rect_source_span(w, h, dw, dh, filter, x0, y0, x1, y1, lx, hx, ly, hy);
            axis_source_span(cfilter, dw, w, x0, x1, clx, chx);
            axis_source_span(cfilter, dh, h, y0, y1, cly, chy);
            g_chroma_wider += clx < lx || chx > hx || cly < ly || chy > hy;
            g_luma_wider += lx < clx || hx > chx || ly < cly || hy > chy;
            const unsigned ux0 = std::min(lx, clx), ux1 = std::max(hx, chx), uy0 = std::min(ly, cly), uy1 = std::max(hy, chy);
            CHECK(xs[c].lo == ux0 && xs[c].hi == ux1 && ys[r].lo == uy0 && ys[r].hi == uy1,
                  "tile (%u,%u) of %ux%u -> %ux%u filter %d: [%u,%u) x [%u,%u), not [%u,%u) x [%u,%u)", c, r, w, h, dw, dh, filter, xs[c].lo, xs[c].hi,
                  ys[r].lo, ys[r].hi, ux0, ux1, uy0, uy1);
        }
    // the table image, and the bisection over it against the definition
    std::vector<unsigned> image(delta_span_words(g.cols, g.rows));
    delta_span_image(xs, ys, image.data());
    const unsigned* xlo = image.data();
    const unsigned* xhi = xlo + g.cols;
    const unsigned* ylo = xhi + g.cols;
    const unsigned* yhi = ylo + g.rows;
    for (unsigned x = 0; x < w; ++x) {
        const unsigned c0 = count_le(xhi, g.cols, x), c1 = count_le(xlo, g.cols, x);
        for (unsigned c = 0; c < g.cols; ++c)
            CHECK((c >= c0 && c < c1) == (xs[c].lo <= x && x < xs[c].hi), "column %u, tile column %u of %ux%u -> %ux%u filter %d", x, c, w, h, dw, dh, filter);
    }
    for (unsigned y = 0; y < h; ++y) {
        const unsigned r0 = count_le(yhi, g.rows, y), r1 = count_le(ylo, g.rows, y);
        for (unsigned r = 0; r < g.rows; ++r)
            CHECK((r >= r0 && r < r1) == (ys[r].lo <= y && y < ys[r].hi), "row %u, tile row %u of %ux%u -> %ux%u filter %d", y, r, w, h, dw, dh, filter);
    }
}

// the items of a grid's rects for one layout, into a full-size image of pitched planes at made-up addresses
static void check_items(const std::vector<DeltaRect>& rects, const RgbListLayout& lay, unsigned dw, bool with_conv)
{
    const size_t n = rects.size(), bpp = lay.row_bytes(1);
    RgbDeltaDst d{};
    for (unsigned p = 0; p < lay.planes(); ++p) {
        d.plane[p] = reinterpret_cast<void*>((size_t)0x1000000 * (p + 1));
        d.pitch[p] = lay.row_bytes(dw) + 2 * (p + 1);
    }
    if (with_conv) { d.conv = reinterpret_cast<void*>((size_t)0x9000000); d.conv_pitch = (size_t)lay.bps * dw + 6; }
    std::vector<srcnn_rgb_rect_item> items(n + 1);
    std::memset(items.data(), 0xEE, sizeof(srcnn_rgb_rect_item) * items.size());
    if (n > 0) {
        CHECK(!rgb_delta_items(rects, lay, d, items.data(), n - 1), "cap one short");
        const unsigned char* raw = reinterpret_cast<const unsigned char*>(items.data());
        bool untouched = true;
        for (size_t i = 0; i < sizeof(srcnn_rgb_rect_item) * items.size(); ++i) untouched = untouched && raw[i] == 0xEE;
        CHECK(untouched, "cap one short wrote items");
    }
    CHECK(rgb_delta_items(rects, lay, d, items.data(), n), "cap = n");
    for (size_t k = 0; k < n; ++k) {
        const srcnn_rgb_rect_item& it = items[k];
        CHECK(it.x0 == rects[k].x0 && it.y0 == rects[k].y0 && it.rw == rects[k].rw && it.rh == rects[k].rh, "item %zu", k);
        for (unsigned p = 0; p < 4; ++p) {
            if (p < lay.planes()) {
                CHECK(reinterpret_cast<size_t>(it.dst[p]) == (size_t)0x1000000 * (p + 1) + (size_t)it.y0 * d.pitch[p] + bpp * it.x0 && it.dst_pitch[p] == d.pitch[p],
                      "item %zu plane %u (bpp %zu) points at %p", k, p, bpp, it.dst[p]);
            } else {
                CHECK(it.dst[p] == nullptr && it.dst_pitch[p] == 0, "item %zu: unused plane %u is set", k, p);
            }
        }
        if (with_conv) CHECK(reinterpret_cast<size_t>(it.dst_conv) == (size_t)0x9000000 + (size_t)it.y0 * d.conv_pitch + (size_t)lay.bps * it.x0 && it.dst_conv_pitch == d.conv_pitch, "item %zu conv", k);
        else CHECK(it.dst_conv == nullptr && it.dst_conv_pitch == 0, "item %zu: conv without a conv plane", k);
    }
    const unsigned char* last = reinterpret_cast<const unsigned char*>(&items[n]);
    CHECK(last[0] == 0xEE && last[sizeof(srcnn_rgb_rect_item) - 1] == 0xEE, "item n was written");
    RgbDeltaDst none = d;
    for (unsigned p = 0; p < 4; ++p) none.plane[p] = nullptr;
    none.conv = nullptr;
    CHECK(rgb_delta_items(rects, lay, none, items.data(), n + 1), "NULL image");
    for (size_t k = 0; k < n; ++k)
        CHECK(items[k].dst[0] == nullptr && items[k].dst[lay.planes() - 1] == nullptr && items[k].dst_conv == nullptr && items[k].dst_pitch[0] == d.pitch[0], "NULL image, item %zu", k);
}

int main()
{
    // ---- span tables: w, h, dw, dh, tile ----
    const unsigned shapes[][6] = {
        {96, 56, 192, 112, 32, 16}, {96, 56, 192, 112, 40, 24},     // 2x, the grids of the issue
        {37, 23, 74, 46, 16, 16},
        {96, 56, 240, 140, 64, 64}, {96, 56, 240, 140, 0, 0},       // 2.5x, and the default tile
        {40, 31, 60, 46, 8, 8}, {40, 31, 60, 46, 16, 24},           // 1.5x
        {24, 24, 24, 24, 8, 8},                                     // the identity size: both axes copied
        {96, 56, 96, 112, 32, 16}, {96, 56, 192, 56, 32, 16},       // one axis keeps its size
        {30, 1, 45, 1, 8, 8},
        {50, 30, 37, 22, 8, 8}, {50, 30, 37, 22, 16, 9},            // a down-scale (0.75x)
        {5, 3, 333, 95, 8, 9},                                      // a steep up-scale: many tiles per source pixel
        {1, 1, 20, 9, 64, 64}, {7, 300, 14, 600, 64, 8},
    };
    for (int filter = 0; filter < 5; ++filter)
        for (const auto& s : shapes) check_spans(s[0], s[1], s[2], s[3], filter, s[4], s[5]);
    // the union is a union: each part reaches past the other somewhere (otherwise min / max would be decoration)
    CHECK(g_luma_wider > 0, "the Y path's span never reaches past the chroma taps'");
    std::printf("tiles where the chroma taps reach past the Y path's span: %u; the other way round: %u\n", g_chroma_wider, g_luma_wider);

    // ---- the items, for every bytes-per-pixel class ----
    std::vector<unsigned char> flags = {0, 1, 1, 0, 0, 1,
                                        0, 1, 1, 0, 0, 0,
                                        1, 0, 0, 0, 1, 1,
                                        0, 0, 0, 0, 1, 1,
                                        0, 0, 0, 0, 0, 0,
                                        1, 1, 1, 1, 1, 1,
                                        0, 0, 0, 0, 0, 1};
    std::vector<DeltaRect> rects;
    CHECK(delta_coalesce(flags.data(), 6, 7, 32, 16, 192, 112, rects) == 6, "%zu rects", rects.size());
    const RgbListLayout layouts[] = {{1, 3, false}, {1, 4, false}, {2, 3, false}, {2, 4, false}, {1, 3, true}, {1, 4, true}, {2, 3, true}, {2, 4, true}};
    const size_t want_bpp[] = {3, 4, 6, 8, 1, 1, 2, 2};
    for (size_t k = 0; k < sizeof layouts / sizeof layouts[0]; ++k) {
        CHECK(layouts[k].row_bytes(1) == want_bpp[k], "layout %zu: %zu bytes per pixel", k, layouts[k].row_bytes(1));
        check_items(rects, layouts[k], 192, true);
        check_items(rects, layouts[k], 192, false);
        check_items(std::vector<DeltaRect>{}, layouts[k], 192, true);
        check_items(std::vector<DeltaRect>{DeltaRect{0, 0, 192, 112}}, layouts[k], 192, k % 2 == 0);
    }

    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
