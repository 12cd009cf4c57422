// yuv_rect_sanitize.cpp -- CPU-only sanitizer harness for the host half of the YUV rect call (include/srcnn_amd_yuv_rect.h):
// no GPU, no HIP.  Built and run by tests/test_yuv_rect_sanitizer.py with -fsanitize=address,undefined, the way `make asan`
// builds tests/host/host_sanitize.cpp.  What runs under the sanitizers:
//   * libsrcnn_amd/csrc/srcnn_rect_source.hpp   srcnn_yuv_rect_source's body (yuv_rect_source) for every plane of every format
//     family over multipliers 0.75 ... 3, all five filters and rect edges at and next to the borders; every result lies inside
//     its plane, plane 0 is the Y path's rectangle, plane 2 of a semi-planar frame is empty;
//   * libsrcnn_amd/csrc/srcnn_frame_args.hpp    check_yuv_rect_args, the argument half of srcnn_yuv_upscale_rect_dev: odd
//     origins, rects outside the output, sums that wrap in 32 bits, pitches, odd addresses, and the end-of-plane pointer
//     arithmetic of the overlap rules -- a rect repainted inside the surface it is read from, two planes of the rect over each
//     other -- on host buffers, with the sizes written out here;
//   * libsrcnn_amd/csrc/srcnn_window_tile.h     window_tile_fits, the predicate that sends a rect's chroma through the fused tile
//     kernels (k_rgb_window_merge, k_yuv_window_chroma) or down the plane route, on tables from build_axis_table: true for every
//     chroma table of an up-scale, false for more than 8 taps, for tables without host copies and for a tile span beyond the patch.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/srcnn_amd.h"
#include "../../include/srcnn_amd_yuv_ex.h"
#include "../../libsrcnn_amd/csrc/srcnn_rect_source.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_window_tile.h"

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

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Format { int layout, chroma, depth, msb; };
static const Format kFormats[] = {
    {SRCNN_YUV_PLANAR, SRCNN_YUV_420, 8, 0}, {SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_420, 8, 0}, {SRCNN_YUV_PLANAR, SRCNN_YUV_422, 10, 0},
    {SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_420, 10, 1}, {SRCNN_YUV_PLANAR, SRCNN_YUV_444, 16, 0}, {SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_444, 12, 1},
    {SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_422, 14, 0}};

static std::vector<unsigned> edges(unsigned n)
{
    const long long c[] = {0, 1, 2, 5, 6, 7, 8, 15, 16, 17, 63, 64, 65, (long long)n - 8, (long long)n - 7, (long long)n - 6, (long long)n - 2,
                           (long long)n - 1, n, n / 2};
    std::vector<unsigned> v;
    for (long long e : c)
        if (e >= 0 && e <= (long long)n) v.push_back((unsigned)e);
    return v;
}

static unsigned ccols(const Format& f, unsigned w) { return f.chroma == SRCNN_YUV_444 ? w : (w + 1) / 2; }
static unsigned crows(const Format& f, unsigned h) { return f.chroma == SRCNN_YUV_420 ? (h + 1) / 2 : h; }

static void check_source_rects()
{
    const unsigned sizes[][2] = {{70, 40}, {35, 21}, {50, 30}, {1, 17}};
    const float muls[] = {0.75f, 1.f, 1.5f, 2.f, 2.5f, 3.f};
    long n = 0;
    for (const Format& f : kFormats) {
        const srcnn_yuv_format fmt = {sizeof(srcnn_yuv_format), f.layout, f.chroma, f.depth, f.msb};
        const bool evx = f.chroma != SRCNN_YUV_444, evy = f.chroma == SRCNN_YUV_420;
        for (auto& sz : sizes)
            for (float mul : muls)
                for (int filter = 0; filter < 5; ++filter) {
                    const unsigned w = sz[0], h = sz[1];
                    unsigned dw = 0, dh = 0;
                    if (srcnn_output_size(w, h, mul, 0, &dw, &dh) != 0) continue;
                    const std::vector<unsigned> ex = edges(dw), ey = edges(dh);
                    for (size_t i = 0; i < ex.size(); ++i)
                        for (size_t j = 0; j < ey.size(); ++j) {
                            // a rect from edge i to a later edge, rows likewise; the pairing rotates so that every edge starts and ends one
                            const unsigned x0 = ex[i], x1 = ex[(i + 1 + (j + filter) % ex.size()) % ex.size()];
                            const unsigned y0 = ey[j], y1 = ey[(j + 1 + (i + filter) % ey.size()) % ey.size()];
                            if (x1 <= x0 || y1 <= y0) continue;
                            const bool odd = (evx && (x0 & 1)) || (evy && (y0 & 1));
                            unsigned r[3][4];
                            for (int plane = 0; plane < 3; ++plane) {
                                const int rc = srcnn::yuv_rect_source(&fmt, w, h, mul, filter, x0, y0, x1 - x0, y1 - y0, plane, &r[plane][0], &r[plane][1],
                                                                      &r[plane][2], &r[plane][3]);
                                CHECK(rc == (odd ? SRCNN_E_ARG : SRCNN_OK), "rect (%u,%u)-(%u,%u) plane %d: %d", x0, y0, x1, y1, plane, rc);
                            }
                            if (odd) continue;
                            ++n;
                            CHECK(r[0][2] > 0 && r[0][3] > 0 && r[0][0] + r[0][2] <= w && r[0][1] + r[0][3] <= h, "luma source outside %ux%u", w, h);
                            unsigned lx, hx, ly, hy;
                            srcnn::y_path_rect_source_span(w, h, dw, dh, filter, x0, y0, x1, y1, lx, hx, ly, hy);
                            CHECK(r[0][0] == lx && r[0][1] == ly && r[0][2] == hx - lx && r[0][3] == hy - ly, "plane 0 is not the Y path's rectangle");
                            const unsigned cw = ccols(f, w), ch = crows(f, h);
                            CHECK(r[1][2] > 0 && r[1][3] > 0 && r[1][0] + r[1][2] <= cw && r[1][1] + r[1][3] <= ch,
                                  "chroma source %ux%u at (%u,%u) outside %ux%u", r[1][2], r[1][3], r[1][0], r[1][1], cw, ch);
                            if (f.layout == SRCNN_YUV_SEMIPLANAR) CHECK(r[2][0] == 0 && r[2][1] == 0 && r[2][2] == 0 && r[2][3] == 0, "plane 2 of a semi-planar frame");
                            else CHECK(memcmp(r[1], r[2], sizeof r[1]) == 0, "U and V differ");
                            if (dw == w && dh == h) {       // the identity size: chroma is copied, its source is the chroma rect
                                const unsigned cx0 = evx ? x0 / 2 : x0, cx1 = evx ? (x1 + 1) / 2 : x1, cy0 = evy ? y0 / 2 : y0, cy1 = evy ? (y1 + 1) / 2 : y1;
                                CHECK(r[1][0] == cx0 && r[1][1] == cy0 && r[1][2] == cx1 - cx0 && r[1][3] == cy1 - cy0, "identity chroma source");
                            }
                        }
                }
        // NULL results, planes outside 0..2, the wrap of x0 + rw
        CHECK(srcnn::yuv_rect_source(&fmt, 8, 8, 2.f, 2, 2, 2, 3, 4, 1, nullptr, nullptr, nullptr, nullptr) == SRCNN_OK, "NULL results");
        unsigned a;
        CHECK(srcnn::yuv_rect_source(&fmt, 8, 8, 2.f, 2, 2, 2, 3, 4, 3, &a, &a, &a, &a) == SRCNN_E_ARG, "plane 3");
        CHECK(srcnn::yuv_rect_source(&fmt, 8, 8, 2.f, 2, 2, 2, 3, 4, -1, &a, &a, &a, &a) == SRCNN_E_ARG, "plane -1");
        CHECK(srcnn::yuv_rect_source(&fmt, 8, 8, 2.f, 2, 0xfffffffeu, 0, 4, 1, 0, &a, &a, &a, &a) == SRCNN_E_ARG, "x0 + rw wraps");
        CHECK(srcnn::yuv_rect_source(&fmt, 8, 8, 2.f, 2, 0, 0xfffffffeu, 1, 4, 0, &a, &a, &a, &a) == SRCNN_E_ARG, "y0 + rh wraps");
        CHECK(srcnn::yuv_rect_source(&fmt, 8, 8, 0.f, 2, 0, 0, 1, 1, 0, &a, &a, &a, &a) == SRCNN_E_SCALE, "scale");
    }
    CHECK(srcnn::yuv_rect_source(nullptr, 8, 8, 2.f, 2, 0, 0, 1, 1, 0, nullptr, nullptr, nullptr, nullptr) == SRCNN_E_ARG, "NULL format");
    CHECK(n > 10000, "only %ld rects", n);
}

// One frame and one rect in ONE host block, each plane exactly as large as the call may touch: the checker's end-of-plane
// arithmetic is then pointer arithmetic inside (or one past) an allocation.
struct Block {
    std::vector<unsigned char> mem;
    void* src[3] = {nullptr, nullptr, nullptr};
    void* dst[3] = {nullptr, nullptr, nullptr};
    size_t src_size[3] = {0, 0, 0}, dst_size[3] = {0, 0, 0};
};

static Block lay_out(const Format& f, unsigned w, unsigned h, unsigned rw, unsigned rh)
{
    Block b;
    const int np = f.layout == SRCNN_YUV_SEMIPLANAR ? 2 : 3;
    const size_t bps = f.depth == 8 ? 1 : 2, spp = np == 2 ? 2 : 1;
    size_t total = 0;
    for (int k = 0; k < np; ++k) {
        b.src_size[k] = k == 0 ? bps * w * h : bps * spp * ccols(f, w) * crows(f, h);
        b.dst_size[k] = k == 0 ? bps * rw * rh : bps * spp * ccols(f, rw) * crows(f, rh);
        b.src_size[k] += b.src_size[k] & 1;
        b.dst_size[k] += b.dst_size[k] & 1;
        total += b.src_size[k] + b.dst_size[k];
    }
    b.mem.assign(total + 2, 0);
    unsigned char* p = b.mem.data();
    p += reinterpret_cast<uintptr_t>(p) & 1;
    for (int k = 0; k < np; ++k) { b.src[k] = p; p += b.src_size[k]; }
    for (int k = 0; k < np; ++k) { b.dst[k] = p; p += b.dst_size[k]; }
    return b;
}

static void check_rect_args()
{
    using srcnn::YuvPlane;
    for (const Format& f : kFormats) {
        const srcnn_yuv_format fmt = {sizeof(srcnn_yuv_format), f.layout, f.chroma, f.depth, f.msb};
        srcnn::YuvGeom g;
        CHECK(srcnn::yuv_geom_from_format(&fmt, g) == SRCNN_OK, "format");
        const int np = g.semi ? 2 : 3;
        const bool evx = f.chroma != SRCNN_YUV_444, evy = f.chroma == SRCNN_YUV_420;
        const unsigned w = 9, h = 7, x0 = 2, y0 = 2, rw = 9, rh = 7;         // -> 18 x 14
        Block b = lay_out(f, w, h, rw, rh);
        unsigned dw = 0, dh = 0;
        YuvPlane in[3], out[3];
        auto call = [&](unsigned X0, unsigned Y0, unsigned RW, unsigned RH, void* const* src, const size_t* sp, void* const* dst, const size_t* dp) {
            return srcnn::check_yuv_rect_args(g, w, h, 2.f, 2, src, sp, X0, Y0, RW, RH, dst, dp, dw, dh, in, out);
        };
        CHECK(call(x0, y0, rw, rh, b.src, nullptr, b.dst, nullptr) == SRCNN_OK && dw == 18 && dh == 14, "the valid call");
        for (int k = 0; k < np; ++k) {                       // what the checker made of the planes, against the sizes written out above
            CHECK(in[k].lo == b.src[k] && (size_t)(in[k].hi() - in[k].lo) + ((in[k].hi() - in[k].lo) & 1) == b.src_size[k], "input plane %d", k);
            CHECK(out[k].lo == b.dst[k] && (size_t)(out[k].hi() - out[k].lo) + ((out[k].hi() - out[k].lo) & 1) == b.dst_size[k], "output plane %d", k);
        }
        // origins
        CHECK(call(3, 2, rw, rh, b.src, nullptr, b.dst, nullptr) == (evx ? SRCNN_E_ARG : SRCNN_OK), "odd x0");
        CHECK(call(2, 3, rw, rh, b.src, nullptr, b.dst, nullptr) == (evy ? SRCNN_E_ARG : SRCNN_OK), "odd y0");
        // the rect's place
        CHECK(call(10, 2, rw, rh, b.src, nullptr, b.dst, nullptr) == SRCNN_E_ARG && call(2, 8, rw, rh, b.src, nullptr, b.dst, nullptr) == SRCNN_E_ARG, "outside");
        CHECK(call(0xfffffffeu, 2, 4, rh, b.src, nullptr, b.dst, nullptr) == SRCNN_E_ARG, "x0 + rw wraps");
        CHECK(call(2, 0xfffffffcu, rw, 6, b.src, nullptr, b.dst, nullptr) == SRCNN_E_ARG, "y0 + rh wraps");
        CHECK(call(2, 2, 0, rh, b.src, nullptr, b.dst, nullptr) == SRCNN_E_ARG && call(2, 2, rw, 0, b.src, nullptr, b.dst, nullptr) == SRCNN_E_ARG, "empty");
        CHECK(call(2, 2, rw, rh, nullptr, nullptr, b.dst, nullptr) == SRCNN_E_ARG && call(2, 2, rw, rh, b.src, nullptr, nullptr, nullptr) == SRCNN_E_ARG, "NULL arrays");
        // pitches: one below the row, per plane and side
        for (int k = 0; k < np; ++k) {
            size_t sp[3] = {0, 0, 0}, dp[3] = {0, 0, 0};
            sp[k] = in[k].row_bytes - g.bps;
            CHECK(call(x0, y0, rw, rh, b.src, sp, b.dst, nullptr) == SRCNN_E_ARG, "short input pitch %d", k);
            dp[k] = out[k].row_bytes - g.bps;
            CHECK(call(x0, y0, rw, rh, b.src, nullptr, b.dst, dp) == SRCNN_E_ARG, "short output pitch %d", k);
            if (g.bps == 2) {
                void* d2[3] = {b.dst[0], b.dst[1], b.dst[2]};
                d2[k] = static_cast<unsigned char*>(d2[k]) + 1;
                CHECK(call(x0, y0, rw, rh, b.src, nullptr, d2, nullptr) == SRCNN_E_ARG, "odd address %d", k);
            }
        }
        // a plane of the rect on the first and on the last byte pair of every input plane, and planes of the rect over each other
        for (int a = 0; a < np; ++a)
            for (int k = 0; k < np; ++k) {
                void* d2[3] = {b.dst[0], b.dst[1], b.dst[2]};
                d2[k] = b.src[a];
                CHECK(call(x0, y0, rw, rh, b.src, nullptr, d2, nullptr) == SRCNN_E_ARG, "output %d on input %d", k, a);
                d2[k] = static_cast<unsigned char*>(b.src[a]) + b.src_size[a] - 2;
                CHECK(call(x0, y0, rw, rh, b.src, nullptr, d2, nullptr) == SRCNN_E_ARG, "output %d on the end of input %d", k, a);
                if (k > a) {
                    d2[k] = b.dst[a];
                    CHECK(call(x0, y0, rw, rh, b.src, nullptr, d2, nullptr) == SRCNN_E_ARG, "outputs %d and %d", a, k);
                }
            }
        // repainting inside the surface the frame is read from (identity size: the surface has the output's size)
        {
            const unsigned W = 16, H = 12;
            Block s = lay_out(f, W, H, 1, 1);
            const size_t spp = g.semi ? 2 : 1;
            size_t pitch[3] = {(size_t)g.bps * W, (size_t)g.bps * spp * g.ccols(W), g.semi ? 0 : (size_t)g.bps * g.ccols(W)};
            void* d2[3] = {nullptr, nullptr, nullptr};
            d2[0] = static_cast<unsigned char*>(s.src[0]) + 2 * pitch[0] + 4 * g.bps;
            for (int k = 1; k < np; ++k) d2[k] = static_cast<unsigned char*>(s.src[k]) + (size_t)(2 >> g.sy) * pitch[k] + (size_t)(4 >> g.sx) * g.bps * spp;
            unsigned ow = 0, oh = 0;
            YuvPlane i2[3], o2[3];
            CHECK(srcnn::check_yuv_rect_args(g, W, H, 1.f, 2, s.src, nullptr, 4, 2, 6, 4, d2, pitch, ow, oh, i2, o2) == SRCNN_E_ARG && ow == W && oh == H,
                  "a rect inside its own source surface");
        }
    }
}

static srcnn::TileAxis tile_axis(const srcnn::AxisTable& t) { return srcnn::TileAxis{t.first.data(), t.taps.data(), t.max_taps}; }

// The route predicate.  Nothing observable says which route a rect took (both give the same bytes at the same cost), so a
// predicate that refused everything would pass every other test: this is where it is held to its answers.
static void check_window_tile_fits()
{
    using srcnn::build_axis_table;
    using srcnn::window_tile_fits;
    const float muls[] = {1.5f, 2.f, 2.5f, 3.f};
    const unsigned lens[] = {9, 70, 97, 1920};
    long n = 0;
    for (int filter : {SRCNN_FILTER_NEAREST, SRCNN_FILTER_BILINEAR})         // (the only filters chroma_filter yields)
        for (float mul : muls)
            for (unsigned lh : lens)
                for (unsigned lv : lens) {
                    const unsigned dh = (unsigned)((float)lh * mul), dv = (unsigned)((float)lv * mul);
                    const srcnn::AxisTable th = build_axis_table(filter, dh, lh), tv = build_axis_table(filter, dv, lv);
                    CHECK(th.max_taps <= 8 && tv.max_taps <= 8, "filter %d x%g: %d / %d taps", filter, mul, th.max_taps, tv.max_taps);
                    CHECK(window_tile_fits(tile_axis(th), tile_axis(tv), 0, dh, 0, dv), "filter %d x%g %ux%u: the whole output", filter, mul, lh, lv);
                    // a rect that starts mid-tile and ends at the far border: its tiles straddle those of the whole output
                    const unsigned x0 = dh > 37 ? 37 : dh / 2, y0 = dv > 5 ? 5 : dv / 2;
                    CHECK(window_tile_fits(tile_axis(th), tile_axis(tv), x0, dh - x0, y0, dv - y0), "filter %d x%g %ux%u: rect at (%u,%u)", filter, mul,
                          lh, lv, x0, y0);
                    n += 2;
                }
    CHECK(n == 2 * 2 * 4 * 4 * 4, "%ld predicate calls", n);
    const srcnn::AxisTable up = build_axis_table(SRCNN_FILTER_BILINEAR, 140, 70);
    CHECK(window_tile_fits(tile_axis(up), tile_axis(up), 0, 140, 0, 140), "2x bilinear");
    // more than 8 taps, in either axis: a 0.25x Lanczos table (whatever its spans)
    const srcnn::AxisTable wide = build_axis_table(SRCNN_FILTER_LANCZOS3, 64, 256);
    CHECK(wide.max_taps > 8, "0.25x Lanczos has %d taps", wide.max_taps);
    CHECK(!window_tile_fits(tile_axis(wide), tile_axis(up), 0, 64, 0, 140) && !window_tile_fits(tile_axis(up), tile_axis(wide), 0, 140, 0, 64), "max_taps > 8");
    srcnn::TileAxis many = tile_axis(up);
    many.max_taps = 9;
    CHECK(!window_tile_fits(many, tile_axis(up), 0, 140, 0, 140) && !window_tile_fits(tile_axis(up), many, 0, 140, 0, 140), "max_taps = 9 alone");
    // no host copies
    const srcnn::TileAxis none = {nullptr, nullptr, up.max_taps}, no_first = {nullptr, up.taps.data(), up.max_taps}, no_taps = {up.first.data(), nullptr, up.max_taps};
    for (const srcnn::TileAxis& bad : {none, no_first, no_taps})
        CHECK(!window_tile_fits(bad, tile_axis(up), 0, 140, 0, 140) && !window_tile_fits(tile_axis(up), bad, 0, 140, 0, 140), "NULL host arrays");
    // a down-scale whose tile span exceeds the patch although its taps are few: 0.5x bilinear (5 taps; 64 outputs read about 130
    // inputs, 16 about 34) and 0.25x nearest (1 tap; 64 outputs read about 253).  0.25x bilinear is refused as well, already for
    // its 9 taps.
    for (const srcnn::AxisTable& down : {build_axis_table(SRCNN_FILTER_BILINEAR, 960, 1920), build_axis_table(SRCNN_FILTER_NEAREST, 480, 1920)}) {
        CHECK(down.max_taps <= 8, "filter %d to %u: %d taps", down.filter, down.dst_len, down.max_taps);
        CHECK(!window_tile_fits(tile_axis(down), tile_axis(up), 0, down.dst_len, 0, 140), "columns to %u: 64 of them span more than %d", down.dst_len, srcnn::kPatchW);
        CHECK(!window_tile_fits(tile_axis(up), tile_axis(down), 0, 140, 0, down.dst_len), "rows to %u: 16 of them span more than %d", down.dst_len, srcnn::kPatchH);
        // ... and one tile of it alone already does, where a tile of the up-scale does not
        CHECK(!srcnn::axis_tiles_fit(down.first.data(), down.taps.data(), down.max_taps, 64, 64, srcnn::kTileW, srcnn::kPatchW), "one tile to %u", down.dst_len);
    }
    CHECK(srcnn::axis_tiles_fit(up.first.data(), up.taps.data(), up.max_taps, 64, 64, srcnn::kTileW, srcnn::kPatchW), "one 2x tile");
    const srcnn::AxisTable quarter = build_axis_table(SRCNN_FILTER_BILINEAR, 480, 1920);
    CHECK(!window_tile_fits(tile_axis(quarter), tile_axis(up), 0, 480, 0, 140) && !window_tile_fits(tile_axis(up), tile_axis(quarter), 0, 140, 0, 480), "0.25x bilinear");
    // an empty range asks nothing of the tables' contents
    CHECK(window_tile_fits(tile_axis(up), tile_axis(up), 10, 0, 10, 0), "empty range");
}

int main()
{
    check_source_rects();
    check_rect_args();
    check_window_tile_fits();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
