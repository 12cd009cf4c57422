// delta_sanitize.cpp -- CPU-only sanitizer harness for the host half of the delta call (include/srcnn_amd_delta.h): no GPU, no
// HIP.  Built and run by tests/test_delta_sanitizer.py with -fsanitize=address,undefined, the way
// tests/test_yuv_rect_list_sanitizer.py builds its program.  What runs under the sanitizers is libsrcnn_amd/csrc/srcnn_delta.hpp:
// the grid (delta_grid), the span-table builder (delta_axis_spans, delta_spans_monotone, delta_span_image), the coalescer
// (delta_coalesce, delta_items), the whole-frame rule (delta_whole_frame), what the *_rects entry points refuse about a stated grid
// (check_delta_tiles) and the plan of a whole operation (delta_plan).  It asserts that
//   * the span of every tile column and row, built from ONE table per axis, is the rectangle y_path_rect_source_span gives for
//     that tile on its own, for all five filters over the grids of the issue, a 2.5x frame, an axis that keeps its size and a
//     down-scale, and that both ends are monotone -- what the kernel's bisection rests on;
//   * the tiles the bisection finds for a source sample are exactly the tiles whose span holds it;
//   * the coalescer's rects are pairwise disjoint, cover exactly the dirty tiles clipped to dw x dh, and follow the rule (a run
//     continues the open rect of the previous row only when its columns are identical), on seeded grids, on the hand cases and on
//     degenerate grids (1 x 1, a 1-tile column, a 1-tile row);
//   * delta_items writes nothing when the capacity is one short, and exactly n items otherwise;
//   * every clause of the whole-frame rule;
//   * check_delta_tiles refuses in its order -- scaled size, tile side, cover -- and accepts cols and rows at exactly the ceiling;
//   * delta_plan yields, branch by branch, the rects and the srcnn_delta_stats of the whole operation: nothing dirty, one change
//     (the two points tests/test_gpu_delta.py::test_canary_repaint pins on the device), every tile dirty, no previous frame, the
//     cells at the threshold and one below it; the rect count is clamped to 32 bits.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../libsrcnn_amd/csrc/srcnn_delta.hpp"

using namespace srcnn;

// The product's fail() lives in srcnn_capi.cpp; this one formats as well, so the sanitizers see every message's arguments.
static char g_last[512];      // the last message
namespace srcnn {
int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last, sizeof g_last, fmt, ap);
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

struct Rng {      // splitmix64: the grids are the same on every machine
    unsigned long long s;
    unsigned long long next() { unsigned long long z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    unsigned below(unsigned n) { return (unsigned)(next() % n); }
};

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

static void check_spans(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, unsigned tile_w, unsigned tile_h, unsigned want_cols, unsigned want_rows)
{
    DeltaGrid g;
    CHECK(delta_grid(w, h, dw, dh, filter, tile_w, tile_h, g) == SRCNN_OK, "%ux%u -> %ux%u", w, h, dw, dh);
    if (want_cols) CHECK(g.cols == want_cols && g.rows == want_rows, "%u x %u, not %u x %u", g.cols, g.rows, want_cols, want_rows);
    std::vector<DeltaSpan> xs, ys;
    delta_axis_spans(filter, dw, w, g.tile_w, xs);
    delta_axis_spans(filter, dh, h, g.tile_h, ys);
    CHECK(xs.size() == g.cols && ys.size() == g.rows, "table sizes");
    CHECK(delta_spans_monotone(xs, w) && delta_spans_monotone(ys, h), "%ux%u -> %ux%u filter %d tile %ux%u", w, h, dw, dh, filter, g.tile_w, g.tile_h);
    for (unsigned r = 0; r < g.rows; ++r)
        for (unsigned c = 0; c < g.cols; ++c) {
            const unsigned x0 = c * g.tile_w, y0 = r * g.tile_h, x1 = std::min(dw, x0 + g.tile_w), y1 = std::min(dh, y0 + g.tile_h);
            unsigned lx, hx, ly, hy;
            y_path_rect_source_span(w, h, dw, dh, filter, x0, y0, x1, y1, lx, hx, ly, hy);
            CHECK(xs[c].lo == lx && xs[c].hi == hx && ys[r].lo == ly && ys[r].hi == hy, "tile (%u,%u) of %ux%u -> %ux%u filter %d: [%u,%u) x [%u,%u), not [%u,%u) x [%u,%u)",
                  c, r, w, h, dw, dh, filter, xs[c].lo, xs[c].hi, ys[r].lo, ys[r].hi, lx, hx, ly, hy);
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

// the properties of the rects of a grid, and the rule restated row by row
static unsigned check_coalesce(const std::vector<unsigned char>& flags, unsigned cols, unsigned rows, unsigned tile_w, unsigned tile_h, unsigned dw, unsigned dh)
{
    std::vector<DeltaRect> rects;
    const unsigned n = delta_coalesce(flags.data(), cols, rows, tile_w, tile_h, dw, dh, rects);
    CHECK(n == rects.size(), "count");
    std::vector<int> paint((size_t)cols * rows, -1);      // which rect covers a tile
    for (unsigned k = 0; k < n; ++k) {
        const DeltaRect& r = rects[k];
        CHECK(r.rw > 0 && r.rh > 0 && r.x0 + r.rw <= dw && r.y0 + r.rh <= dh, "rect %u: %ux%u at (%u,%u) in %ux%u", k, r.rw, r.rh, r.x0, r.y0, dw, dh);
        CHECK(r.x0 % tile_w == 0 && r.y0 % tile_h == 0, "rect %u starts off the grid", k);
        CHECK(((r.x0 + r.rw) % tile_w == 0 || r.x0 + r.rw == dw) && ((r.y0 + r.rh) % tile_h == 0 || r.y0 + r.rh == dh), "rect %u ends off the grid", k);
        const unsigned c0 = r.x0 / tile_w, c1 = (r.x0 + r.rw + tile_w - 1) / tile_w, r0 = r.y0 / tile_h, r1 = (r.y0 + r.rh + tile_h - 1) / tile_h;
        for (unsigned rr = r0; rr < r1 && rr < rows; ++rr)
            for (unsigned c = c0; c < c1 && c < cols; ++c) {
                CHECK(paint[(size_t)rr * cols + c] < 0, "tile (%u,%u) is covered twice", c, rr);
                paint[(size_t)rr * cols + c] = (int)k;
            }
        // maximal: the tiles left and right of every row of the rect are clean or outside
        for (unsigned rr = r0; rr < r1 && rr < rows; ++rr) {
            CHECK(c0 == 0 || !flags[(size_t)rr * cols + c0 - 1], "rect %u is not a maximal run on its left", k);
            CHECK(c1 >= cols || !flags[(size_t)rr * cols + c1], "rect %u is not a maximal run on its right", k);
        }
    }
    for (unsigned rr = 0; rr < rows; ++rr)
        for (unsigned c = 0; c < cols; ++c) {
            CHECK((paint[(size_t)rr * cols + c] >= 0) == (flags[(size_t)rr * cols + c] != 0), "tile (%u,%u): dirty %d, covered %d", c, rr, flags[(size_t)rr * cols + c], paint[(size_t)rr * cols + c]);
            // the rule: the same rect as the tile above exactly when the run above has the same columns
            if (rr && flags[(size_t)rr * cols + c] && flags[(size_t)(rr - 1) * cols + c]) {
                unsigned a = c, b = c, a2 = c, b2 = c;
                while (a > 0 && flags[(size_t)rr * cols + a - 1]) --a;
                while (b + 1 < cols && flags[(size_t)rr * cols + b + 1]) ++b;
                while (a2 > 0 && flags[(size_t)(rr - 1) * cols + a2 - 1]) --a2;
                while (b2 + 1 < cols && flags[(size_t)(rr - 1) * cols + b2 + 1]) ++b2;
                CHECK((paint[(size_t)rr * cols + c] == paint[(size_t)(rr - 1) * cols + c]) == (a == a2 && b == b2), "tile (%u,%u): continuation", c, rr);
            }
        }
    // the items: one short writes nothing, enough writes n
    float* const base = reinterpret_cast<float*>(0x100000);
    const size_t pitch = sizeof(float) * dw + 64;
    std::vector<srcnn_rect_item> items(n + 1);
    std::memset(items.data(), 0xEE, sizeof(srcnn_rect_item) * items.size());
    if (n > 0) {
        CHECK(!delta_items(rects, base, pitch, items.data(), n - 1), "cap one short");
        const unsigned char* raw = reinterpret_cast<const unsigned char*>(items.data());
        bool untouched = true;
        for (size_t i = 0; i < sizeof(srcnn_rect_item) * items.size(); ++i) untouched = untouched && raw[i] == 0xEE;
        CHECK(untouched, "cap one short wrote items");
    }
    CHECK(delta_items(rects, base, pitch, items.data(), n), "cap = n");
    for (unsigned k = 0; k < n; ++k) {
        const srcnn_rect_item& it = items[k];
        CHECK(it.x0 == rects[k].x0 && it.y0 == rects[k].y0 && it.rw == rects[k].rw && it.rh == rects[k].rh && it.out_pitch == pitch, "item %u", k);
        CHECK(reinterpret_cast<size_t>(it.d_out) == 0x100000 + (size_t)it.y0 * pitch + sizeof(float) * it.x0, "item %u points at %p", k, (void*)it.d_out);
    }
    const unsigned char* last = reinterpret_cast<const unsigned char*>(&items[n]);
    CHECK(last[0] == 0xEE && last[sizeof(srcnn_rect_item) - 1] == 0xEE, "item n was written");
    CHECK(delta_items(rects, nullptr, pitch, items.data(), n + 1) && (n == 0 || items[0].d_out == nullptr), "NULL d_out");
    return n;
}

static std::vector<unsigned char> grid_of(unsigned cols, unsigned rows, const char* rows_text)
{
    std::vector<unsigned char> f((size_t)cols * rows, 0);
    size_t i = 0;
    for (const char* p = rows_text; *p; ++p)
        if (*p == '#' || *p == '.') { if (i < f.size()) f[i] = *p == '#'; ++i; }
    CHECK(i == f.size(), "grid text has %zu cells, not %zu", i, f.size());
    return f;
}

// check_delta_tiles refuses with `code` and a message that holds `what`
static bool refuses(int rc, int code, const char* what) { return rc == code && std::strstr(g_last, what); }

// the plan of the 6 x 7 grid of 32 x 16 tiles over 192 x 112 (text: grid_of's, NULL: no previous frame)
static srcnn_delta_stats plan_of(const char* text, long permille, std::vector<DeltaRect>& rects)
{
    const DeltaGrid g{32, 16, 6, 7};
    std::vector<unsigned char> f;
    if (text) f = grid_of(6, 7, text);
    srcnn_delta_stats st;
    std::memset(&st, 0xEE, sizeof st);
    rects.assign(3, DeltaRect{9, 9, 9, 9});              // (what the call's vector held before does not matter)
    delta_plan(text ? f.data() : nullptr, g, 192, 112, permille, st, rects);
    CHECK(st.struct_size == sizeof(srcnn_delta_stats), "struct_size %u", st.struct_size);
    return st;
}
static bool stats_are(const srcnn_delta_stats& s, unsigned tiles, unsigned dirty, unsigned rects, unsigned whole, unsigned long long cells)
{
    return s.tiles == tiles && s.dirty_tiles == dirty && s.rects == rects && s.whole_frame == whole && s.cell_samples == cells;
}
static bool is_rect(const DeltaRect& r, unsigned x0, unsigned y0, unsigned rw, unsigned rh) { return r.x0 == x0 && r.y0 == y0 && r.rw == rw && r.rh == rh; }

int main()
{
    // ---- span tables ----
    for (int filter = 0; filter < 5; ++filter) {
        check_spans(96, 56, 192, 112, filter, 32, 16, 6, 7);
        check_spans(96, 56, 192, 112, filter, 40, 24, 5, 5);
        check_spans(37, 23, 74, 46, filter, 16, 16, 5, 3);
        check_spans(96, 56, 240, 140, filter, 64, 64, 4, 3);       // 2.5x
        check_spans(96, 56, 240, 140, filter, 0, 0, 4, 3);         // the defaults
        check_spans(96, 56, 96, 112, filter, 32, 16, 3, 7);        // the columns keep their size
        check_spans(96, 56, 192, 56, filter, 32, 16, 6, 4);        // the rows do
        check_spans(50, 30, 37, 20, filter, 8, 8, 5, 3);           // a down-scale
        check_spans(9, 7, 18, 14, filter, 8, 8, 3, 2);
        check_spans(5, 3, 333, 95, filter, 8, 9, 42, 11);          // a steep up-scale: many tiles per source sample
        check_spans(1, 1, 20, 9, filter, 64, 64, 1, 1);            // 1 x 1
        check_spans(7, 300, 14, 600, filter, 64, 8, 1, 75);        // a 1-tile column
    }
    // ---- the grid's rules ----
    DeltaGrid g;
    CHECK(delta_grid(0, 5, 10, 10, 2, 0, 0, g) == SRCNN_E_ARG && delta_grid(5, 5, 0, 10, 2, 0, 0, g) == SRCNN_E_SCALE && delta_grid(5, 5, 10, 10, 5, 0, 0, g) == SRCNN_E_ARG, "grid rules");
    CHECK(delta_grid(5, 5, 10, 10, 2, 7, 0, g) == SRCNN_E_ARG && delta_grid(5, 5, 10, 10, 2, 0, 65536, g) == SRCNN_E_ARG, "tile rules");
    CHECK(delta_grid(5, 5, 8 * 2048, 10, 2, 8, 8, g) == SRCNN_OK && g.cols == 2048 && delta_grid(5, 5, 8 * 2048 + 1, 10, 2, 8, 8, g) == SRCNN_E_UNSUPPORTED, "grid limit");
    CHECK(delta_grid(5, 5, 0x7fffff, 65535 * 16, 2, 65535, 65535, g) == SRCNN_OK && delta_grid(5, 5, 0x800000, 10, 2, 65535, 65535, g) == SRCNN_E_UNSUPPORTED, "Y path limits");

    // ---- the coalescer: hand cases on the 6 x 7 grid of 32 x 16 tiles over 192 x 112 ----
    const unsigned C6 = 6, R7 = 7;
    CHECK(check_coalesce(grid_of(C6, R7, "...... ...... ...... ...... ...... ...... ......"), C6, R7, 32, 16, 192, 112) == 0, "empty");
    CHECK(check_coalesce(grid_of(C6, R7, "###### ###### ###### ###### ###### ###### ######"), C6, R7, 32, 16, 192, 112) == 1, "full");
    CHECK(check_coalesce(grid_of(C6, R7, "...... ...... ...... ..#... ...... ...... ......"), C6, R7, 32, 16, 192, 112) == 1, "one tile");
    CHECK(check_coalesce(grid_of(C6, R7, "...... .#.... .#.... .#.... .###.. ...... ......"), C6, R7, 32, 16, 192, 112) == 2, "an L");
    CHECK(check_coalesce(grid_of(C6, R7, "#.#.#. .#.#.# #.#.#. .#.#.# #.#.#. .#.#.# #.#.#."), C6, R7, 32, 16, 192, 112) == 21, "checkerboard");
    CHECK(check_coalesce(grid_of(C6, R7, "...... ...... ##.### ##.##. ...... ...... ......"), C6, R7, 32, 16, 192, 112) == 3, "two runs, one continues");
    CHECK(check_coalesce(grid_of(C6, R7, ".##... ...... .##... ...... ...... ...... ......"), C6, R7, 32, 16, 192, 112) == 2, "the same run after a clean row");
    CHECK(check_coalesce(grid_of(5, 5, "##### ##### ##### ##### #####"), 5, 5, 40, 24, 192, 112) == 1, "partial last tiles");
    CHECK(check_coalesce(grid_of(5, 5, "..... ..... ..... ..... ....#"), 5, 5, 40, 24, 192, 112) == 1, "the partial corner");
    // degenerate grids
    CHECK(check_coalesce(grid_of(1, 1, "#"), 1, 1, 64, 64, 20, 9) == 1 && check_coalesce(grid_of(1, 1, "."), 1, 1, 64, 64, 20, 9) == 0, "1 x 1");
    CHECK(check_coalesce(grid_of(1, 4, "# . # #"), 1, 4, 64, 8, 10, 30) == 2, "a 1-tile column");
    CHECK(check_coalesce(grid_of(5, 1, "##.#."), 5, 1, 8, 64, 37, 9) == 2, "a 1-tile row");
    // ---- seeded grids ----
    Rng rng{20260};
    const unsigned shapes[][4] = {{32, 16, 192, 112}, {40, 24, 192, 112}, {16, 16, 74, 46}, {64, 64, 240, 140}, {8, 8, 333, 95}, {8, 8, 2048, 16}, {8, 8, 16, 2048}};
    for (const auto& s : shapes) {
        const unsigned cols = (s[2] + s[0] - 1) / s[0], rows = (s[3] + s[1] - 1) / s[1];
        for (unsigned density = 1; density < 10; density += 2)
            for (int rep = 0; rep < 4; ++rep) {
                std::vector<unsigned char> f((size_t)cols * rows);
                for (auto& v : f) v = rng.below(10) < density ? (unsigned char)(1 + rng.below(255)) : 0;
                check_coalesce(f, cols, rows, s[0], s[1], s[2], s[3]);
            }
    }

    // ---- the whole-frame rule: 192 x 112 = 21504 samples, 42 tiles ----
    CHECK(!delta_whole_frame(0, 0, 42, 0, 192, 112, 1000), "nothing changed");
    CHECK(!delta_whole_frame(0, 0, 42, 0, 192, 112, 0), "nothing changed, whatever the switch");
    CHECK(delta_whole_frame(1, 42, 42, 204 * 124, 192, 112, 1000000), "every tile dirty");
    CHECK(!delta_whole_frame(1, 6, 42, 4560, 192, 112, 1000), "one 64 x 48 rect: 21 %% of the frame");
    CHECK(delta_whole_frame(1, 6, 42, 4560, 192, 112, 212) && !delta_whole_frame(1, 6, 42, 4560, 192, 112, 213), "the share is reached, not exceeded: 4560 / 21504 = 0.21205");
    CHECK(delta_whole_frame(3, 30, 42, 21504, 192, 112, 1000) && !delta_whole_frame(3, 30, 42, 21503, 192, 112, 1000), "at 1000 the cells equal the frame");
    CHECK(delta_whole_frame(65537, 65537, 1u << 20, 65537ull * 20 * 20, 7680, 8 << 20 >> 10, 1000000), "more rects than a list holds");
    CHECK(!delta_whole_frame(65536, 65536, 1u << 20, 65536ull * 400, 7680, 8192, 1000), "65536 rects are a list");
    std::vector<DeltaRect> two = {{64, 32, 64, 48}, {0, 0, 64, 32}};
    CHECK(delta_cell_samples(two) == 4560 + 3344, "cell samples");

    // ---- a stated grid: each refusal in order, then the accepted edges ----
    CHECK(refuses(check_delta_tiles(9, 9, 7, 7, 0, 112), SRCNN_E_SCALE, "scaled size") && refuses(check_delta_tiles(9, 9, 7, 7, 192, 0), SRCNN_E_SCALE, "scaled size"), "the size first");
    CHECK(refuses(check_delta_tiles(9, 9, 7, 16, 192, 112), SRCNN_E_ARG, "a side is") && refuses(check_delta_tiles(9, 9, 32, 65536, 192, 112), SRCNN_E_ARG, "a side is") &&
          refuses(check_delta_tiles(9, 9, 0, 16, 192, 112), SRCNN_E_ARG, "a side is"), "then the tile, 0 included: no default here");
    CHECK(refuses(check_delta_tiles(5, 7, 32, 16, 192, 112), SRCNN_E_ARG, "do not cover") && refuses(check_delta_tiles(7, 7, 32, 16, 192, 112), SRCNN_E_ARG, "do not cover") &&
          refuses(check_delta_tiles(6, 6, 32, 16, 192, 112), SRCNN_E_ARG, "do not cover") && refuses(check_delta_tiles(6, 8, 32, 16, 192, 112), SRCNN_E_ARG, "do not cover"), "then the cover");
    CHECK(check_delta_tiles(6, 7, 32, 16, 192, 112) == SRCNN_OK && check_delta_tiles(5, 5, 40, 24, 192, 112) == SRCNN_OK, "cols and rows at the ceiling, whole and partial last tiles");
    CHECK(check_delta_tiles(24, 14, 8, 8, 192, 112) == SRCNN_OK && check_delta_tiles(1, 1, 65535, 65535, 192, 112) == SRCNN_OK, "the smallest and the largest tile");

    // ---- the plan of a whole operation, branch by branch (850: the default of SRCNN_DELTA_WHOLE_PERMILLE) ----
    std::vector<DeltaRect> rects;
    CHECK(stats_are(plan_of("...... ...... ...... ...... ...... ...... ......", 850, rects), 42, 0, 0, 0, 0) && rects.empty(), "nothing dirty: no rects, not the whole frame");
    // the two points of tests/test_gpu_delta.py::test_canary_repaint, from the flags its restatement expects
    CHECK(stats_are(plan_of("...... ...... ..##.. ..##.. ..##.. ...... ......", 850, rects), 42, 6, 1, 0, 4560) && rects.size() == 1 && is_rect(rects[0], 64, 32, 64, 48), "a change at (48, 28)");
    CHECK(stats_are(plan_of("##.... ##.... ...... ...... ...... ...... ......", 850, rects), 42, 4, 1, 0, 3344) && rects.size() == 1 && is_rect(rects[0], 0, 0, 64, 32), "a change at (20, 10)");
    CHECK(stats_are(plan_of("...... ...... ...... ..#... ...... ...... ......", 850, rects), 42, 1, 1, 0, 44 * 28) && rects.size() == 1 && is_rect(rects[0], 64, 48, 32, 16), "one tile");
    CHECK(stats_are(plan_of("###### ###### ###### ###### ###### ###### ######", 1000000, rects), 42, 42, 1, 1, 204 * 124) && rects.size() == 1 && is_rect(rects[0], 0, 0, 192, 112),
          "every tile dirty, whatever the switch");
    CHECK(stats_are(plan_of(nullptr, 1000000, rects), 42, 42, 1, 1, 204 * 124) && rects.size() == 1 && is_rect(rects[0], 0, 0, 192, 112), "no previous frame: as if every tile were dirty");
    // 4560 / 21504 = 0.21205: reached at 212, not at 213; the rects collapse to the one, the stats keep what the coalescer gave
    CHECK(stats_are(plan_of("...... ...... ..##.. ..##.. ..##.. ...... ......", 212, rects), 42, 6, 1, 1, 4560) && rects.size() == 1 && is_rect(rects[0], 0, 0, 192, 112), "at the threshold");
    CHECK(stats_are(plan_of("...... ...... ..##.. ..##.. ..##.. ...... ......", 213, rects), 42, 6, 1, 0, 4560) && rects.size() == 1 && is_rect(rects[0], 64, 32, 64, 48), "one below it");
    CHECK(stats_are(plan_of("##.... ##.... ..##.. ..##.. ..##.. ...... ......", 367, rects), 42, 10, 2, 1, 7904) && rects.size() == 1 && is_rect(rects[0], 0, 0, 192, 112), "7904 / 21504 = 0.36756, two rects");
    CHECK(stats_are(plan_of("##.... ##.... ..##.. ..##.. ..##.. ...... ......", 368, rects), 42, 10, 2, 0, 7904) && rects.size() == 2 && is_rect(rects[0], 0, 0, 64, 32) && is_rect(rects[1], 64, 32, 64, 48),
          "two rects, in the order they were opened");
    CHECK(delta_rect_count(0) == 0 && delta_rect_count(65537) == 65537 && delta_rect_count((size_t)0xffffffffu) == 0xffffffffu &&
          delta_rect_count((size_t)0xffffffffu + 1) == 0xffffffffu && delta_rect_count((size_t)1 << 40) == 0xffffffffu, "the rect count is clamped to 32 bits");

    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
