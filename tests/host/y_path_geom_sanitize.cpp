// y_path_geom_sanitize.cpp -- CPU-only sanitizer harness for the Y path's geometry (libsrcnn_amd/csrc/srcnn_y_path_geom.hpp): no
// GPU, no HIP.  Built and run by tests/test_y_path_geom_sanitizer.py with -fsanitize=address,undefined, the way
// tests/test_delta_sanitizer.py builds its program.  Every function of the header is held against a restatement that shares
// none of its text:
//   * y_path_halo, for every len in 1..24 and every 0 <= a < b <= len, against set dilation: [a,b) marked in a bool[len], grown
//     by 2 with clipping (ca, cb), then by 4 (ua, ub);
//   * taps_span, over the tables of build_axis_table for all five filters and the axes 7->13, 13->7, 16->32, 5->23 and 9->9,
//     for every a < b, against a literal min / max over first[u] and first[u] + taps[u], cut at src_len;
//   * y_path_band_rows against the rule as the four call sites used to spell it, at the cases that decide it: the exact fit, one
//     byte short of it, a budget under the 16-row floor, the fused tier with no budget at all, fewer rows than the band -- and
//     over a sweep of budgets around every one of them;
//   * y_path_fits at each limit and one past it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../libsrcnn_amd/csrc/resample_table.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_y_path_geom.hpp"

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

// every index within r of a marked one, inside [0, len)
static std::vector<bool> dilate(const std::vector<bool>& in, int r)
{
    const int len = (int)in.size();
    std::vector<bool> out(in.size(), false);
    for (int i = 0; i < len; ++i)
        if (in[i])
            for (int j = i - r; j <= i + r; ++j)
                if (j >= 0 && j < len) out[j] = true;
    return out;
}
static void bounds(const std::vector<bool>& m, unsigned& lo, unsigned& hi)
{
    lo = hi = 0;
    bool any = false;
    for (size_t i = 0; i < m.size(); ++i)
        if (m[i]) { if (!any) lo = (unsigned)i; any = true; hi = (unsigned)i + 1; }
}

static void check_halo()
{
    static_assert(kConv3Halo == (5 - 1) / 2 && kConv1Halo == (9 - 1) / 2, "the halos of a 5x5 and a 9x9 layer");
    for (unsigned len = 1; len <= 24; ++len)
        for (unsigned a = 0; a < len; ++a)
            for (unsigned b = a + 1; b <= len; ++b) {
                std::vector<bool> m(len, false);
                for (unsigned i = a; i < b; ++i) m[i] = true;
                const std::vector<bool> c = dilate(m, 2), u = dilate(c, 4);
                unsigned ca, cb, ua, ub;
                bounds(c, ca, cb);
                bounds(u, ua, ub);
                const HaloSpan s = y_path_halo(len, a, b);
                CHECK(s.ca == ca && s.cb == cb && s.ua == ua && s.ub == ub, "len %u [%u,%u): [%u,%u) [%u,%u), dilation gives [%u,%u) [%u,%u)", len, a, b,
                      s.ca, s.cb, s.ua, s.ub, ca, cb, ua, ub);
                CHECK(s.width() == ub - ua, "len %u [%u,%u): width %u", len, a, b, s.width());
            }
}

static void check_taps_span()
{
    const unsigned axes[5][2] = {{7, 13}, {13, 7}, {16, 32}, {5, 23}, {9, 9}};      // src_len -> dst_len
    for (int filter = 0; filter <= 4; ++filter)
        for (const auto& ax : axes) {
            const unsigned src_len = ax[0], dst_len = ax[1];
            const AxisTable t = build_axis_table(filter, dst_len, src_len);
            for (unsigned a = 0; a < dst_len; ++a)
                for (unsigned b = a + 1; b <= dst_len; ++b) {
                    long mn = 1L << 40, mx = -1;
                    for (unsigned u = a; u < b; ++u) {
                        if (t.first[u] < mn) mn = t.first[u];
                        if ((long)t.first[u] + t.taps[u] > mx) mx = (long)t.first[u] + t.taps[u];
                    }
                    if (mx > (long)src_len) mx = src_len;
                    unsigned lo = ~0u, hi = ~0u;
                    taps_span(t.first.data(), t.taps.data(), src_len, a, b, lo, hi);
                    CHECK((long)lo == mn && (long)hi == mx, "filter %d, %u -> %u, [%u,%u): [%u,%u), the table says [%ld,%ld)", filter, src_len, dst_len, a, b, lo,
                          hi, mn, mx);
                    CHECK(lo < hi && hi <= src_len, "filter %d, %u -> %u, [%u,%u): [%u,%u) is empty or outside the axis", filter, src_len, dst_len, a, b, lo, hi);
                }
        }
}

// the rule as y_path_range, y_path_rect, y_path_rect_band_rows and yuv_band_rows each spelled it, with budget_band_rows inlined
static unsigned band_rule(size_t budget, bool fused, unsigned W, unsigned rows)
{
    const size_t row_bytes = (size_t)32 * W * sizeof(float);
    if (fused) return rows;
    if (row_bytes * ((size_t)rows + 4) <= budget) return rows;
    size_t fit = budget / row_bytes;
    size_t band = fit > 4 ? fit - 4 : 1;
    if (band < 16) band = 16;
    if (band > (1u << 20)) band = 1u << 20;
    return rows < band ? rows : (unsigned)band;
}

static void check_band()
{
    const unsigned W = 74, rows = 106;
    const size_t row_bytes = (size_t)32 * 4 * W, fit = row_bytes * (rows + 4);
    CHECK(y_path_band_rows(fit, false, W, rows) == rows, "the exact fit is one pass: %u", y_path_band_rows(fit, false, W, rows));
    CHECK(y_path_band_rows(fit - 1, false, W, rows) == rows - 1, "one byte short: 110 rows no longer fit, 109 - 4 do: %u", y_path_band_rows(fit - 1, false, W, rows));
    CHECK(y_path_band_rows(row_bytes * 19, false, W, rows) == 16, "19 rows' worth: the 16-row floor, not 15: %u", y_path_band_rows(row_bytes * 19, false, W, rows));
    CHECK(y_path_band_rows(1, false, W, rows) == 16, "a budget below one row: the floor: %u", y_path_band_rows(1, false, W, rows));
    CHECK(y_path_band_rows(0, false, W, rows) == 16, "no budget: the floor: %u", y_path_band_rows(0, false, W, rows));
    CHECK(y_path_band_rows(0, true, W, rows) == rows, "the fused tier has no planes: one pass whatever the budget: %u", y_path_band_rows(0, true, W, rows));
    CHECK(y_path_band_rows(0, false, W, 7) == 7, "fewer rows than the band: %u", y_path_band_rows(0, false, W, 7));
    CHECK(y_path_band_rows(row_bytes * 40, false, W, 30) == 30, "30 rows under a band of 36: %u", y_path_band_rows(row_bytes * 40, false, W, 30));
    CHECK(y_path_band_rows(row_bytes * 40, false, W, 37) == 36, "37 rows under a band of 36: %u", y_path_band_rows(row_bytes * 40, false, W, 37));
    // the wrapper budget_band_rows(dw) asks for 1 << 20 rows: the cap of a band, reached or not
    CHECK(y_path_band_rows(~(size_t)0, false, 1, 1u << 20) == 1u << 20, "the cap");
    CHECK(y_path_band_rows((size_t)128 * ((1u << 20) + 3), false, 1, 1u << 20) == (1u << 20) - 1, "one row under the cap");
    for (unsigned w : {1u, 13u, 74u, 421u, 7680u})
        for (unsigned r : {1u, 15u, 16u, 17u, 40u, 106u, 4320u}) {
            const size_t rb = (size_t)128 * w;
            for (size_t k : {(size_t)0, (size_t)1, (size_t)4, (size_t)5, (size_t)19, (size_t)20, (size_t)21, (size_t)r, (size_t)r + 3, (size_t)r + 4, (size_t)r + 5})
                for (long d = -1; d <= 1; ++d) {
                    if (k == 0 && d < 0) continue;
                    const size_t budget = rb * k + (size_t)d;
                    for (int fused = 0; fused <= 1; ++fused)
                        CHECK(y_path_band_rows(budget, fused != 0, w, r) == band_rule(budget, fused != 0, w, r), "budget %zu, fused %d, W %u, rows %u: %u, the rule says %u",
                              budget, fused, w, r, y_path_band_rows(budget, fused != 0, w, r), band_rule(budget, fused != 0, w, r));
                }
        }
}

static void check_limits()
{
    const unsigned M = 1u << 20;
    CHECK(y_path_fits(0x7fffffffULL, M, 0x7fffffu, M, 65535u * 16u), "every limit reached, none passed");
    CHECK(!y_path_fits(0x80000000ULL, M, 0x7fffffu, M, 65535u * 16u), "2^31 source samples");
    CHECK(!y_path_fits(0, M + 1, 1, 1, 1), "2^20 + 1 source rows");
    CHECK(!y_path_fits(0, 1, 0x800000u, 1, 1), "2^23 output columns");
    CHECK(!y_path_fits(0, 1, 1, M + 1, 1), "2^20 + 1 output rows");
    CHECK(!y_path_fits(0, 1, 1, M, 65535u * 16u + 1), "one row more than a launch's grid covers");
    CHECK(y_path_fits(0, 1, 1, 1, 1), "the smallest frame");
}

int main()
{
    check_halo();
    check_taps_span();
    check_band();
    check_limits();
    if (g_fail) { std::printf("%d checks FAILED\n", g_fail); return 1; }
    std::printf("y_path_geom: all checks passed\n");
    return 0;
}
