// yuv_packed_rect_sanitize.cpp -- CPU-only sanitizer harness for the host half of the packed YUV rect call
// (include/srcnn_amd_yuv_packed_rect.h): no GPU, no HIP.  Built and run by tests/test_yuv_packed_rect_sanitizer.py with
// -fsanitize=address,undefined, the way `make asan` builds tests/host/host_sanitize.cpp.  What runs under the sanitizers:
//   * libsrcnn_amd/csrc/srcnn_rect_source.hpp   the bodies of srcnn_yuv_packed_span_bytes and srcnn_yuv_packed_rect_source for all ten
//     formats over the shapes of tests/test_yuv_packed_rect_abi.py: widths of every residue of the unit and 47 / 48 / 49 / 97 / 140,
//     multipliers 0.75 ... 3, all five filters, rect edges at and next to the borders; every span lies inside its tight row, every
//     source rectangle inside the frame, under the unit rule, and holds the Y path's rectangle;
//   * libsrcnn_amd/csrc/srcnn_frame_args.hpp    check_yuv_packed_rect_args, the argument half of srcnn_yuv_packed_upscale_rect_dev: the
//     unit rule, rects outside the output, sums that wrap in 32 bits, pitches, alignment, and the end-of-frame pointer arithmetic
//     of the overlap rule on host buffers with the sizes written out here;
//   * yuvp_window_fits, the predicate that sends a rect through k_yuvp_window_merge or down the plane route, on tables from
//     build_axis_table, with the tile width v210 really uses (60): true for every chroma table of an up-scale, false for more
//     than 8 taps, for tables without host copies and for a tile span beyond the patch.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/srcnn_amd.h"
#include "../../include/srcnn_amd_yuv_packed.h"
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

// unit in pixels, unit in bytes, alignment: the header's table, written out
static const struct { unsigned unit, bytes, align; } kUnits[10] = {{2, 4, 1}, {2, 4, 1}, {2, 4, 1}, {2, 8, 2}, {2, 8, 2}, {2, 8, 2}, {1, 4, 1}, {1, 4, 4}, {1, 8, 2}, {6, 16, 4}};

static size_t tight(int format, unsigned w)
{
    if (format <= 2) return 4 * (size_t)((w + 1) / 2);
    if (format <= 5) return 8 * (size_t)((w + 1) / 2);
    if (format == 6 || format == 7) return 4 * (size_t)w;
    if (format == 8) return 8 * (size_t)w;
    return 128 * (size_t)((w + 47) / 48);
}

static std::vector<unsigned> edges(unsigned n)
{
    const long long c[] = {0, 1, 2, 5, 6, 7, 8, 15, 16, 17, 63, 64, 65, (long long)n - 8, (long long)n - 7, (long long)n - 6, (long long)n - 2,
                           (long long)n - 1, n, n / 2};
    std::vector<unsigned> v;
    for (long long e : c)
        if (e >= 0 && e <= (long long)n) v.push_back((unsigned)e);
    return v;
}

static void check_spans()
{
    long n = 0;
    for (int format = 0; format < 10; ++format) {
        const unsigned u = kUnits[format].unit;
        std::vector<unsigned> widths = {47, 48, 49, 97, 140};
        for (unsigned w = 1; w <= 3 * u + 1; ++w) widths.push_back(w);
        for (unsigned width : widths) {
            size_t rb = 0;
            unsigned al = 0;
            srcnn::YuvPackedGeom g;
            CHECK(srcnn::yuv_packed_geom(format, g) == SRCNN_OK, "format %d", format);
            rb = g.row_bytes(width); al = g.align;
            CHECK(rb == tight(format, width) && al == kUnits[format].align, "row bytes of %u in format %d", width, format);
            for (unsigned x = 0; x <= width + 1; ++x)
                for (unsigned cnt : {0u, 1u, u, u + 1, 2 * u, width > x ? width - x : 0u, width + 1}) {
                    unsigned unit = 0;
                    size_t off = 0, len = 0;
                    const bool inside = cnt > 0 && (unsigned long long)x + cnt <= width;
                    const bool ok = inside && x % u == 0 && (cnt % u == 0 || x + cnt == width);
                    const int rc = srcnn::yuv_packed_span_bytes(format, width, x, cnt, &unit, &off, &len);
                    CHECK(rc == (ok ? SRCNN_OK : SRCNN_E_ARG), "span [%u,+%u) of %u in format %d: %d", x, cnt, width, format, rc);
                    if (!ok) continue;
                    ++n;
                    CHECK(unit == u && off == (size_t)(x / u) * kUnits[format].bytes && off + len <= rb && len > 0 && len % 4 == 0, "span [%u,+%u) of %u", x, cnt, width);
                    CHECK((x + cnt == width) == (off + len == rb) || (x + cnt) / u * kUnits[format].bytes == rb, "the row's end, [%u,+%u) of %u", x, cnt, width);
                }
            CHECK(srcnn::yuv_packed_span_bytes(format, width, 0, width, nullptr, nullptr, nullptr) == SRCNN_OK, "NULL results");
            CHECK(srcnn::yuv_packed_span_bytes(format, width, 0xfffffffeu, 4, nullptr, nullptr, nullptr) == SRCNN_E_ARG, "x + n wraps");
        }
    }
    CHECK(srcnn::yuv_packed_span_bytes(-1, 8, 0, 8, nullptr, nullptr, nullptr) == SRCNN_E_ARG && srcnn::yuv_packed_span_bytes(10, 8, 0, 8, nullptr, nullptr, nullptr) == SRCNN_E_ARG, "unknown format");
    CHECK(n > 1000, "only %ld spans", n);
}

static void check_source_rects()
{
    const unsigned sizes[][2] = {{70, 40}, {35, 21}, {50, 30}, {1, 17}, {3, 40}};
    const float muls[] = {0.75f, 1.f, 1.5f, 2.f, 2.5f, 3.f};
    long n = 0;
    for (int format = 0; format < 10; ++format) {
        const unsigned u = kUnits[format].unit;
        for (auto& sz : sizes)
            for (float mul : muls)
                for (int filter = 0; filter < 5; ++filter) {
                    const unsigned w = sz[0], h = sz[1];
                    unsigned dw = 0, dh = 0;
                    if (srcnn_output_size(w, h, mul, 0, &dw, &dh) != 0) continue;
                    const std::vector<unsigned> ex = edges(dw), ey = edges(dh);
                    for (size_t i = 0; i < ex.size(); ++i)
                        for (size_t j = 0; j < ey.size(); ++j) {
                            const unsigned x0 = ex[i], x1 = ex[(i + 1 + (j + filter) % ex.size()) % ex.size()];
                            const unsigned y0 = ey[j], y1 = ey[(j + 1 + (i + filter) % ey.size()) % ey.size()];
                            if (x1 <= x0 || y1 <= y0) continue;
                            const bool ok = x0 % u == 0 && ((x1 - x0) % u == 0 || x1 == dw);
                            unsigned r[4] = {0, 0, 0, 0};
                            const int rc = srcnn::yuv_packed_rect_source(format, w, h, mul, filter, x0, y0, x1 - x0, y1 - y0, &r[0], &r[1], &r[2], &r[3]);
                            CHECK(rc == (ok ? SRCNN_OK : SRCNN_E_ARG), "format %d rect (%u,%u)-(%u,%u) of %ux%u: %d", format, x0, y0, x1, y1, dw, dh, rc);
                            if (!ok) continue;
                            ++n;
                            CHECK(r[2] > 0 && r[3] > 0 && r[0] + r[2] <= w && r[1] + r[3] <= h, "source outside %ux%u", w, h);
                            CHECK(r[0] % u == 0 && (r[2] % u == 0 || r[0] + r[2] == w), "source (%u,+%u) of %u breaks the unit rule", r[0], r[2], w);
                            CHECK(srcnn::yuv_packed_span_bytes(format, w, r[0], r[2], nullptr, nullptr, nullptr) == SRCNN_OK, "the source rectangle is no span");
                            unsigned lx, hx, ly, hy;
                            srcnn::y_path_rect_source_span(w, h, dw, dh, filter, x0, y0, x1, y1, lx, hx, ly, hy);
                            CHECK(r[0] <= lx && hx <= r[0] + r[2] && r[1] <= ly && hy <= r[1] + r[3], "the Y path's rectangle is not inside");
                            if (x0 == 0 && x1 == dw && y0 == 0 && y1 == dh) CHECK(r[0] == 0 && r[1] == 0 && r[2] == w && r[3] == h, "a whole-frame rect");
                        }
                }
        unsigned a;
        CHECK(srcnn::yuv_packed_rect_source(format, 12, 8, 2.f, 2, 6, 2, 12, 4, nullptr, nullptr, nullptr, nullptr) == SRCNN_OK, "NULL results");
        CHECK(srcnn::yuv_packed_rect_source(format, 12, 8, 2.f, 2, 0xfffffffau, 0, 12, 1, &a, &a, &a, &a) == SRCNN_E_ARG, "x0 + rw wraps");
        CHECK(srcnn::yuv_packed_rect_source(format, 12, 8, 2.f, 2, 0, 0xfffffffeu, 6, 4, &a, &a, &a, &a) == SRCNN_E_ARG, "y0 + rh wraps");
        CHECK(srcnn::yuv_packed_rect_source(format, 12, 8, 0.f, 2, 1, 0, 1, 1, &a, &a, &a, &a) == SRCNN_E_SCALE, "the scale before the unit rule");
    }
    CHECK(srcnn::yuv_packed_rect_source(10, 8, 8, 2.f, 2, 0, 0, 1, 1, nullptr, nullptr, nullptr, nullptr) == SRCNN_E_ARG, "unknown format");
    CHECK(n > 10000, "only %ld rects", n);
}

static void check_rect_args()
{
    using srcnn::YuvPlane;
    for (int format = 0; format < 10; ++format) {
        srcnn::YuvPackedGeom g;
        CHECK(srcnn::yuv_packed_geom(format, g) == SRCNN_OK, "format %d", format);
        const unsigned u = kUnits[format].unit, al = kUnits[format].align;
        const unsigned w = 12, h = 7, x0 = 6, y0 = 2, rw = 12, rh = 7;        // -> 24 x 14; 6 and 12 suit every unit, and 18 < 24
        const size_t src_size = tight(format, w) * h, seg = (size_t)(rw / u) * kUnits[format].bytes, dst_size = seg * rh;
        // ONE host block, each side exactly as large as the call may touch: the checker's end-of-plane arithmetic is then pointer
        // arithmetic inside (or one past) an allocation
        std::vector<unsigned char> mem(src_size + dst_size + 16);
        unsigned char* src = mem.data() + ((16 - (reinterpret_cast<uintptr_t>(mem.data()) & 15)) & 15);
        unsigned char* dst = src + src_size;
        unsigned dw = 0, dh = 0;
        YuvPlane in, out;
        auto call = [&](unsigned X0, unsigned Y0, unsigned RW, unsigned RH, const void* s, size_t sp, void* d, size_t dp) {
            return srcnn::check_yuv_packed_rect_args(g, w, h, 2.f, 2, s, sp, X0, Y0, RW, RH, d, dp, dw, dh, in, out);
        };
        CHECK(call(x0, y0, rw, rh, src, 0, dst, 0) == SRCNN_OK && dw == 24 && dh == 14, "the valid call");
        CHECK(in.lo == src && (size_t)(in.hi() - in.lo) == src_size && out.lo == dst && (size_t)(out.hi() - out.lo) == dst_size && out.row_bytes == seg, "the sides");
        // the unit rule
        if (u > 1) {
            CHECK(call(x0 + 1, y0, rw, rh, src, 0, dst, 0) == SRCNN_E_ARG, "x0 off the unit");
            CHECK(call(x0, y0, rw - 1, rh, src, 0, dst, 0) == SRCNN_E_ARG, "rw off the unit, short of dw");
        }
        CHECK(call(18, y0, 6, rh, src, 0, dst, 0) == SRCNN_OK && call(18, y0, 5, rh, src, 0, dst, 0) == (u == 1 ? SRCNN_OK : SRCNN_E_ARG) && call(19, y0, 5, rh, src, 0, dst, 0) == (u == 1 ? SRCNN_OK : SRCNN_E_ARG), "rects that end the row");
        // the rect's place
        CHECK(call(18, 2, rw, rh, src, 0, dst, 0) == SRCNN_E_ARG && call(6, 8, rw, rh, src, 0, dst, 0) == SRCNN_E_ARG, "outside");
        CHECK(call(0xfffffffau, 2, 12, rh, src, 0, dst, 0) == SRCNN_E_ARG, "x0 + rw wraps");
        CHECK(call(6, 0xfffffffcu, rw, 6, src, 0, dst, 0) == SRCNN_E_ARG, "y0 + rh wraps");
        CHECK(call(6, 2, 0, rh, src, 0, dst, 0) == SRCNN_E_ARG && call(6, 2, rw, 0, src, 0, dst, 0) == SRCNN_E_ARG, "empty");
        CHECK(call(6, 2, rw, rh, nullptr, 0, dst, 0) == SRCNN_E_ARG && call(6, 2, rw, rh, src, 0, nullptr, 0) == SRCNN_E_ARG, "NULL");
        // pitches and alignment
        CHECK(call(x0, y0, rw, rh, src, tight(format, w) - al, dst, 0) == SRCNN_E_ARG, "short input pitch");
        CHECK(call(x0, y0, rw, rh, src, 0, dst, seg - al) == SRCNN_E_ARG, "short output pitch");
        CHECK(call(x0, y0, rw, rh, src, tight(format, w), dst, seg) == SRCNN_OK, "the span is pitch enough");
        if (al > 1) {
            CHECK(call(x0, y0, rw, rh, src + 1, 0, dst, 0) == SRCNN_E_ARG && call(x0, y0, rw, rh, src, 0, dst + al / 2, 0) == SRCNN_E_ARG, "misaligned base");
            CHECK(call(x0, y0, rw, rh, src, 0, dst, seg + al / 2) == SRCNN_E_ARG, "misaligned pitch");
        }
        // the rect on the first and on the last bytes of the source, and right in front of it
        CHECK(call(x0, y0, rw, rh, src, 0, src, 0) == SRCNN_E_ARG, "output on the input");
        CHECK(call(x0, y0, rw, rh, src, 0, src + src_size - 4, 0) == SRCNN_E_ARG || src_size < 4, "output on the end of the input");
        // repainting inside the surface the frame is read from (identity size)
        {
            const unsigned W = 24, H = 12;
            std::vector<unsigned char> surf(tight(format, W) * H + 16);
            unsigned char* s0 = surf.data() + ((16 - (reinterpret_cast<uintptr_t>(surf.data()) & 15)) & 15);
            size_t off = 0, len = 0;
            srcnn::yuv_packed_span(g.rule.kind, W, 6, 12, off, len);
            unsigned ow = 0, oh = 0;
            YuvPlane i2, o2;
            CHECK(srcnn::check_yuv_packed_rect_args(g, W, H, 1.f, 2, s0, 0, 6, 2, 12, 4, s0 + 2 * tight(format, W) + off, tight(format, W), ow, oh, i2, o2) == SRCNN_E_ARG &&
                  ow == W && oh == H, "a rect inside its own source surface");
        }
    }
}

static srcnn::TileAxis tile_axis(const srcnn::AxisTable& t) { return srcnn::TileAxis{t.first.data(), t.taps.data(), t.max_taps}; }

// The route predicate.  Nothing observable says which route a rect took (both give the same bytes), so a predicate that refused
// everything would pass every other test: this is where it is held to its answers, with both tile widths.
static void check_window_fits()
{
    using srcnn::build_axis_table;
    using srcnn::yuvp_window_fits;
    const int kinds[] = {srcnn::kPk422x8, srcnn::kPk422x16, srcnn::kPk444x8, srcnn::kPk410, srcnn::kPk444x16, srcnn::kPkV210};
    CHECK(srcnn::yuv_packed_tile_cols(srcnn::kPkV210) == 60 && srcnn::yuv_packed_tile_cols(srcnn::kPk422x8) == 64 && srcnn::yuv_packed_tile_cols(srcnn::kPk410) == 64, "tile widths");
    const float muls[] = {1.5f, 2.f, 2.5f, 3.f};
    const unsigned lens[] = {9, 70, 97, 1920};
    long n = 0;
    for (int kind : kinds)
        for (int filter : {SRCNN_FILTER_NEAREST, SRCNN_FILTER_BILINEAR})     // (the only filters chroma_filter yields)
            for (float mul : muls)
                for (unsigned lh : lens)
                    for (unsigned lv : lens) {
                        // the chroma grid of a frame lh x lv scaled by mul: ceil(./2) columns for the 4:2:2 kinds
                        const unsigned step = srcnn::yuv_packed_chroma_step(kind);
                        const unsigned dwl = (unsigned)((float)lh * mul), dv = (unsigned)((float)lv * mul);
                        const unsigned cw = (lh + step - 1) / step, dcw = (dwl + step - 1) / step;
                        if (dcw <= cw) continue;
                        const srcnn::AxisTable th = build_axis_table(filter, dcw, cw), tv = build_axis_table(filter, dv, lv);
                        CHECK(th.max_taps <= 8 && tv.max_taps <= 8, "filter %d x%g: %d / %d taps", filter, mul, th.max_taps, tv.max_taps);
                        CHECK(yuvp_window_fits(kind, tile_axis(th), tile_axis(tv), 0, dcw, 0, dv), "kind %d filter %d x%g %ux%u: the whole output", kind, filter, mul, lh, lv);
                        const unsigned cx0 = dcw > 39 ? 39 : 0, y0 = dv > 5 ? 5 : dv / 2;      // (39: a multiple of 3, a v210 group boundary)
                        CHECK(yuvp_window_fits(kind, tile_axis(th), tile_axis(tv), cx0, dcw - cx0, y0, dv - y0), "kind %d filter %d x%g %ux%u: rect at (%u,%u)", kind,
                              filter, mul, lh, lv, cx0, y0);
                        n += 2;
                    }
    CHECK(n > 2 * 6 * 2 * 4 * 4 * 3, "%ld predicate calls", n);
    const srcnn::AxisTable up = build_axis_table(SRCNN_FILTER_BILINEAR, 140, 70);
    const srcnn::AxisTable wide = build_axis_table(SRCNN_FILTER_LANCZOS3, 64, 256);
    CHECK(wide.max_taps > 8, "0.25x Lanczos has %d taps", wide.max_taps);
    srcnn::TileAxis many = tile_axis(up);
    many.max_taps = 9;
    const srcnn::TileAxis none = {nullptr, nullptr, up.max_taps};
    const srcnn::AxisTable down = build_axis_table(SRCNN_FILTER_BILINEAR, 960, 1920);
    for (int kind : kinds) {
        CHECK(yuvp_window_fits(kind, tile_axis(up), tile_axis(up), 0, 140, 0, 140), "kind %d: 2x bilinear", kind);
        CHECK(!yuvp_window_fits(kind, tile_axis(wide), tile_axis(up), 0, 64, 0, 140) && !yuvp_window_fits(kind, tile_axis(up), tile_axis(wide), 0, 140, 0, 64), "max_taps > 8");
        CHECK(!yuvp_window_fits(kind, many, tile_axis(up), 0, 140, 0, 140) && !yuvp_window_fits(kind, tile_axis(up), many, 0, 140, 0, 140), "max_taps = 9 alone");
        CHECK(!yuvp_window_fits(kind, none, tile_axis(up), 0, 140, 0, 140) && !yuvp_window_fits(kind, tile_axis(up), none, 0, 140, 0, 140), "NULL host arrays");
        CHECK(!yuvp_window_fits(kind, tile_axis(down), tile_axis(up), 0, 960, 0, 140) && !yuvp_window_fits(kind, tile_axis(up), tile_axis(down), 0, 140, 0, 960), "0.5x bilinear");
        CHECK(yuvp_window_fits(kind, tile_axis(up), tile_axis(up), 9, 0, 9, 0), "empty range");
    }
    // the tile width matters: columns whose taps lie 1.2 inputs apart span 73 inputs over 64 outputs and 71 over 60
    {
        std::vector<int> first(256), taps(256, 2);
        for (int i = 0; i < 256; ++i) first[i] = i * 6 / 5;
        const srcnn::TileAxis wideish = {first.data(), taps.data(), 2};
        CHECK((63 * 6 / 5 + 2) > srcnn::kPatchW && (59 * 6 / 5 + 2) <= srcnn::kPatchW, "the hand-made table");
        CHECK(!yuvp_window_fits(srcnn::kPk422x8, wideish, tile_axis(up), 0, 128, 0, 140) && yuvp_window_fits(srcnn::kPkV210, wideish, tile_axis(up), 0, 120, 0, 140),
              "64-column tiles span more than the patch, 60-column tiles do not");
    }
}

int main()
{
    check_spans();
    check_source_rects();
    check_rect_args();
    check_window_fits();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("all checks passed\n");
    return 0;
}
