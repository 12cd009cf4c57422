// host_sanitize.cpp -- CPU-only sanitizer harness for the HOST code of the drop-in (the
// reference has latent out-of-bounds bugs of exactly this class, src/frawscale.cpp:185-193,249).
//
// Built by `make asan` (-fsanitize=address,undefined) and `make tsan` (-fsanitize=thread); no GPU, no HIP.
// What runs under the sanitizers:
//   * libsrcnn_amd/csrc/resample_table.hpp  (the product's contribution-table builder) for all five filters over
//     up-/down-scale ratios incl. 1-pixel axes, checked against the oracle's table bit for bit;
//   * libsrcnn_amd/csrc/dropin.cpp          (ProcessSRCNN / ConfigureFilterSRCNN: argument checks, the step-scaling
//     loop, new[] ownership of intermediates and results) with srcnn_process_u8 -- the one device call it makes --
//     replaced by a stand-in that forwards to the CPU oracle.  The stand-in exists only in this test binary;
//   * oracle/srcnn_oracle.c itself on odd plane shapes;
//   * concurrent ProcessSRCNN calls from 4 threads (the TSan target: the drop-in keeps no per-call state);
//   * libsrcnn_amd/csrc/srcnn_watchdog.hpp  (the deadline around every blocking RCCL call) hammered from 4 threads, some of
//     them toggling the timeout to 0 between calls: regions are exclusive, a no-op arm() never releases somebody else's region,
//     a region that outlives its deadline is marked (under the lock) and aborted exactly once, stale generations are ignored;
//   * libsrcnn_amd/csrc/srcnn_frame_args.hpp (everything the YUV / packed / RGB frame calls decide before any device lookup:
//     plane geometry, pitches, alignment, the end-of-plane pointer arithmetic of the overlap rules) on host buffers;
//   * libsrcnn_amd/csrc/srcnn_owned.hpp      (the two owner types every HIP resource of the host layer is a member of) with
//     malloc-backed traits that count and log their calls: a double or a missing free fails the ASan run by itself.
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <thread>
#include <vector>

#include "../../include/libsrcnn_dropin.h"
#include "../../include/srcnn_amd.h"
#include "../../include/srcnn_amd_debug.h"
#include "../../libsrcnn_amd/csrc/resample_table.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_frame_args.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_owned.hpp"
#include "../../libsrcnn_amd/csrc/srcnn_watchdog.hpp"

extern "C" {
int oracle_axis_window(int filter, unsigned dst_len, unsigned src_len);
void oracle_axis_table(int filter, unsigned dst_len, unsigned src_len, int* left, int* right, double* w);
int oracle_y_path(const float* y, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, float* out, float* up,
                  float* c1, float* c2);
int oracle_dosrcnn(const unsigned char* rgb, unsigned w, unsigned h, unsigned d, float mul, int filter, unsigned char* out,
                   unsigned char* conv_opt);
}

// ---- the stand-in for the device call (test binary only) ----
static std::atomic<int> g_calls{0};
extern "C" int srcnn_process_u8(const unsigned char* rgb, unsigned w, unsigned h, unsigned d, float multiply, int filter,
                                unsigned char* out, unsigned char* conv_opt)
{
    ++g_calls;
    if (d != 3 && d != 4) return SRCNN_E_UNSUPPORTED;
    return oracle_dosrcnn(rgb, w, h, d, multiply, filter, out, conv_opt);
}

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static void check_tables()
{
    const unsigned pairs[][2] = {{1, 1}, {2, 1}, {1, 2}, {7, 3}, {3, 7}, {50, 1}, {1, 50}, {34, 23}, {2160, 1080}, {11, 23},
                                 {512, 256}, {255, 256}, {257, 256}, {9, 600}};
    for (int f = 0; f < 5; ++f)
        for (auto& p : pairs) {
            const unsigned dst = p[0], src = p[1];
            const srcnn::AxisTable t = srcnn::build_axis_table(f, dst, src);
            const int win = oracle_axis_window(f, dst, src);
            CHECK(win == t.window, "window f=%d %u<-%u: %d vs %d", f, dst, src, t.window, win);
            std::vector<int> L(dst), R(dst);
            std::vector<double> Wt((size_t)dst * (win + 1), 0.0);
            oracle_axis_table(f, dst, src, L.data(), R.data(), Wt.data());
            for (unsigned u = 0; u < dst; ++u) {
                CHECK(t.first[u] >= 0 && t.first[u] + t.taps[u] <= (int)src && t.taps[u] >= 1 && t.taps[u] <= t.window,
                      "range f=%d %u<-%u u=%u: first %d taps %d", f, dst, src, u, t.first[u], t.taps[u]);
                CHECK(t.first[u] == L[u] && t.last[u] == R[u], "bounds f=%d %u<-%u u=%u", f, dst, src, u);
                CHECK(memcmp(&t.weight[(size_t)u * t.stride], &Wt[(size_t)u * (win + 1)], sizeof(double) * t.taps[u]) == 0,
                      "weights f=%d %u<-%u u=%u", f, dst, src, u);
            }
        }
}

static void check_oracle_shapes()
{
    const unsigned shapes[][2] = {{1, 1}, {17, 1}, {1, 13}, {31, 29}, {5, 64}};
    for (auto& s : shapes) {
        const unsigned w = s[0], h = s[1];
        std::vector<float> y((size_t)w * h), out((size_t)4 * w * h);
        for (size_t i = 0; i < y.size(); ++i) y[i] = (float)((i * 37) % 256);
        CHECK(oracle_y_path(y.data(), w, h, 2 * w, 2 * h, 2, out.data(), nullptr, nullptr, nullptr) == 0, "y_path %ux%u", w, h);
        for (float v : out) CHECK(std::isfinite(v) && v >= 0.f && v <= 255.f, "range");
    }
}

static std::vector<unsigned char> image(unsigned w, unsigned h, unsigned d, unsigned seed)
{
    std::vector<unsigned char> v((size_t)w * h * d);
    unsigned x = seed * 2654435761u + 1;
    for (auto& b : v) { x = x * 1664525u + 1013904223u; b = (unsigned char)(x >> 24); }
    return v;
}

// what ProcessSRCNN must return for (img, mul, step): the reference's pass structure replayed through the oracle
static std::vector<unsigned char> expected(const std::vector<unsigned char>& img, unsigned w, unsigned h, unsigned d, float mul,
                                           bool step, int filter, unsigned& ow, unsigned& oh)
{
    std::vector<unsigned char> cur = img;
    unsigned cw = w, ch = h;
    auto pass = [&](float f) {
        const unsigned nw = (unsigned)((float)cw * f), nh = (unsigned)((float)ch * f);
        std::vector<unsigned char> nxt((size_t)nw * nh * d);
        oracle_dosrcnn(cur.data(), cw, ch, d, f, filter, nxt.data(), nullptr);
        cur.swap(nxt); cw = nw; ch = nh;
    };
    if (!step) pass(mul);
    else {
        int passes = (int)(mul / 2.f);
        if (fmodf(mul, 2.f) > 0.f) ++passes;
        for (int p = 0; p < passes; ++p) {
            float f = 2.f;
            if (p + 1 == passes) { f = ((float)w * mul) / (float)cw; if (f == 0.f || f == 1.f) break; }
            pass(f);
        }
    }
    ow = cw; oh = ch;
    return cur;
}

static void check_dropin()
{
    unsigned char* out = nullptr; unsigned osz = 0;
    const std::vector<unsigned char> tiny = image(4, 4, 3, 1);
    CHECK(ProcessSRCNN(nullptr, 4, 4, 3, 2.f, out, osz, nullptr, nullptr) == -1, "NULL");
    CHECK(ProcessSRCNN(tiny.data(), 0, 4, 3, 2.f, out, osz, nullptr, nullptr) == -1, "w=0");
    CHECK(ProcessSRCNN(tiny.data(), 4, 4, 0, 2.f, out, osz, nullptr, nullptr) == -1, "d=0");
    CHECK(ProcessSRCNN(tiny.data(), 4, 4, 3, 0.f, out, osz, nullptr, nullptr) == -2, "mul=0");
    CHECK(ProcessSRCNN(tiny.data(), 4, 4, 3, -1.f, out, osz, nullptr, nullptr) == -2, "mul<0");
    CHECK(ProcessSRCNN(tiny.data(), 4, 4, 3, 0.1f, out, osz, nullptr, nullptr) == -2, "scaled size 0");
    CHECK(out == nullptr && g_calls == 0, "no device call / no allocation on the error paths");

    struct Case { unsigned w, h, d; float mul; bool step; int filter; };
    const Case cases[] = {{24, 20, 3, 2.f, false, 2}, {24, 20, 4, 2.f, false, 2}, {13, 9, 3, 1.5f, false, 3}, {10, 7, 4, 3.f, false, 1},
                          {12, 10, 3, 4.f, true, 2}, {12, 10, 3, 3.f, true, 2}, {9, 8, 4, 2.5f, true, 4}, {9, 8, 3, 2.f, true, 0},
                          {1, 1, 3, 2.f, false, 2}, {1, 5, 4, 6.f, true, 2}};
    for (const Case& c : cases) {
        const std::vector<unsigned char> img = image(c.w, c.h, c.d, c.w * 31 + c.h);
        ConfigureFilterSRCNN((SRCNNFilterType)c.filter, c.step);
        unsigned char *o = nullptr, *cv = nullptr; unsigned os = 0, cs = 0;
        const int rc = ProcessSRCNN(img.data(), c.w, c.h, c.d, c.mul, o, os, &cv, &cs);
        unsigned ow = 0, oh = 0, qw = 0, qh = 0;
        const std::vector<unsigned char> want = expected(img, c.w, c.h, c.d, c.mul, c.step, c.filter, ow, oh);
        CHECK(rc == 0, "rc %d for %ux%ux%u x%.1f step=%d", rc, c.w, c.h, c.d, c.mul, (int)c.step);
        CHECK(srcnn_output_size(c.w, c.h, c.mul, c.step, &qw, &qh) == 0 && qw == ow && qh == oh, "output_size %ux%u vs %ux%u", qw, qh, ow, oh);
        CHECK(os == ow * oh * c.d && cs == ow * oh, "sizes %u %u", os, cs);
        CHECK(o && memcmp(o, want.data(), want.size()) == 0, "bytes for %ux%ux%u x%.1f step=%d", c.w, c.h, c.d, c.mul, (int)c.step);
        srcnn_delete_array(o);          // delete[]: ASan's alloc-dealloc-mismatch check pins the new[] contract
        delete[] cv;
        // without the conv-Y out-params
        o = nullptr; os = 0;
        CHECK(ProcessSRCNN(img.data(), c.w, c.h, c.d, c.mul, o, os, nullptr, nullptr) == 0 && os == ow * oh * c.d, "no-conv call");
        delete[] o;
    }
    ConfigureFilterSRCNN(SRCNNF_Bicubic, false);
    // d outside {3,4}: the stand-in (like the product) refuses; nothing may leak
    const std::vector<unsigned char> gray = image(6, 6, 1, 3);
    out = nullptr; osz = 0;
    CHECK(ProcessSRCNN(gray.data(), 6, 6, 1, 2.f, out, osz, nullptr, nullptr) == SRCNN_E_UNSUPPORTED && out == nullptr, "d=1");
}

static void check_threads()
{
    ConfigureFilterSRCNN(SRCNNF_Bicubic, false);
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    for (int t = 0; t < 4; ++t)
        th.emplace_back([t, &bad] {
            const unsigned w = 10 + 3 * t, h = 8 + t, d = 3 + (t & 1);
            const std::vector<unsigned char> img = image(w, h, d, 100 + t);
            unsigned ow, oh;
            const std::vector<unsigned char> want = expected(img, w, h, d, 2.f, false, 2, ow, oh);
            for (int it = 0; it < 8; ++it) {
                unsigned char *o = nullptr, *cv = nullptr; unsigned os = 0, cs = 0;
                if (ProcessSRCNN(img.data(), w, h, d, 2.f, o, os, &cv, &cs) != 0 || os != want.size() || memcmp(o, want.data(), os) != 0) ++bad;
                delete[] o; delete[] cv;
                unsigned char* e = nullptr; unsigned es = 0;
                if (ProcessSRCNN(nullptr, w, h, d, 2.f, e, es, nullptr, nullptr) != -1) ++bad;      // argument-check path
            }
        });
    for (auto& t : th) t.join();
    CHECK(bad == 0, "%d concurrent calls went wrong", bad.load());
}

static void check_watchdog()
{
    // (everything the watchdog's detached thread can touch lives for ever, as in the product, where the watchdog is a leaked singleton)
    static std::atomic<int> marks{0}, aborts{0}, inside{0}, overlap{0};
    static std::atomic<unsigned> current_gen{1};
    static srcnn::Watchdog& wd = *new srcnn::Watchdog([](unsigned gen) { if (gen == current_gen.load()) ++marks; },
                                                      [](void*, unsigned gen) { if (gen == current_gen.load()) ++aborts; });
    std::atomic<int> timeout{30};
    std::atomic<int> fired_seen{0}, slow_regions{0};
    auto worker = [&](int id) {
        for (int it = 0; it < 200; ++it) {
            if (id == 3 && (it % 7) == 0) timeout = timeout.load() ? 0 : 30;          // a thread that switches the deadline off and on
            int dummy = 0;
            const bool armed = wd.arm(&dummy, current_gen.load(), timeout.load());
            if (armed) {
                if (inside.fetch_add(1) != 0) ++overlap;                              // armed regions must be exclusive
                const bool slow = id == 0 && (it % 50) == 49;                         // a "blocked RCCL call": outlives its deadline
                if (slow) { ++slow_regions; std::this_thread::sleep_for(std::chrono::milliseconds(80)); }
                inside.fetch_sub(1);
            }
            if (wd.disarm(armed)) ++fired_seen;
        }
    };
    std::vector<std::thread> th;
    for (int i = 0; i < 4; ++i) th.emplace_back(worker, i);
    for (auto& t : th) t.join();
    std::this_thread::sleep_for(std::chrono::milliseconds(50));
    CHECK(overlap.load() == 0, "watchdog: %d overlapping armed regions", overlap.load());
    CHECK(fired_seen.load() == slow_regions.load(), "watchdog: %d regions outlived their deadline, %d saw it", slow_regions.load(), fired_seen.load());
    CHECK(marks.load() == slow_regions.load() && aborts.load() == slow_regions.load(), "watchdog: marks %d aborts %d for %d slow regions",
          marks.load(), aborts.load(), slow_regions.load());
    // a stale generation: the region was armed for communicator generation 1, the communicator is replaced while it blocks
    int dummy = 0;
    const int m0 = marks.load(), a0 = aborts.load();
    const bool armed = wd.arm(&dummy, 1, 20);
    current_gen = 2;
    std::this_thread::sleep_for(std::chrono::milliseconds(60));
    CHECK(wd.disarm(armed), "watchdog: the stale region's deadline still fires for its owner");
    CHECK(marks.load() == m0 && aborts.load() == a0, "watchdog: a stale generation must not touch the new communicator");
}

// ---- the argument half of the frame calls (srcnn_frame_args.hpp) ----
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

using srcnn::YuvPlane;

// One checker behind one signature.  np planes per side; with conv the RGB call's dst_conv rides as dst[np] / dp[np] / out[np].
struct Family {
    const char* name;
    int np;
    bool conv;
    unsigned align;          // of base and pitch
    bool out_out;            // output planes over each other are refused (the RGB call only)
    std::function<int(unsigned w, unsigned h, float mul, int filter, void* const* src, const size_t* sp, void* const* dst,
                      const size_t* dp, YuvPlane* in, YuvPlane* out)> check;
    int nout() const { return np + (conv ? 1 : 0); }
};

static std::vector<Family> frame_families()
{
    std::vector<Family> v;
    const struct { int layout, chroma, depth, msb; } yuv[] = {
        {SRCNN_YUV_PLANAR, SRCNN_YUV_420, 8, 0}, {SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_420, 8, 0}, {SRCNN_YUV_PLANAR, SRCNN_YUV_422, 10, 0},
        {SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_420, 10, 1}, {SRCNN_YUV_PLANAR, SRCNN_YUV_444, 16, 0}, {SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_444, 12, 1}};
    for (auto& f : yuv) {
        const srcnn_yuv_format fmt = {sizeof(srcnn_yuv_format), f.layout, f.chroma, f.depth, f.msb};
        srcnn::YuvGeom g;
        CHECK(srcnn::yuv_geom_from_format(&fmt, g) == SRCNN_OK, "yuv format");
        v.push_back({"yuv", g.semi ? 2 : 3, false, g.bps, false,
                     [g](unsigned w, unsigned h, float mul, int filter, void* const* src, const size_t* sp, void* const* dst, const size_t* dp,
                         YuvPlane* in, YuvPlane* out) {
                         unsigned dw = 0, dh = 0;
                         return srcnn::check_yuv_args(g, w, h, mul, filter, src, sp, dst, dp, dw, dh, in, out);
                     }});
    }
    for (int format = SRCNN_YUVP_YUY2; format <= SRCNN_YUVP_V210; ++format) {
        srcnn::YuvPackedGeom g;
        CHECK(srcnn::yuv_packed_geom(format, g) == SRCNN_OK, "packed format %d", format);
        v.push_back({"packed", 1, false, g.align, false,
                     [g](unsigned w, unsigned h, float mul, int filter, void* const* src, const size_t* sp, void* const* dst, const size_t* dp,
                         YuvPlane* in, YuvPlane* out) {
                         unsigned dw = 0, dh = 0;
                         return srcnn::check_yuv_packed_args(g, w, h, mul, filter, src ? src[0] : nullptr, sp ? sp[0] : 0, dst ? dst[0] : nullptr,
                                                             dp ? dp[0] : 0, dw, dh, in[0], out[0]);
                     }});
    }
    const struct { int layout, order, alpha, depth; bool conv; } rgb[] = {
        {SRCNN_RGB_INTERLEAVED, SRCNN_RGB_ORDER_RGB, 0, 8, true}, {SRCNN_RGB_INTERLEAVED, SRCNN_RGB_ORDER_BGR, 1, 12, true},
        {SRCNN_RGB_PLANAR, SRCNN_RGB_ORDER_RGB, 1, 10, true}, {SRCNN_RGB_PLANAR, SRCNN_RGB_ORDER_BGR, 0, 8, false}};
    for (auto& f : rgb) {
        const srcnn_rgb_format fmt = {sizeof(srcnn_rgb_format), f.layout, f.order, f.alpha, f.depth};
        srcnn::RgbRule g;
        CHECK(srcnn::rgb_rule_from_format(&fmt, g) == SRCNN_OK, "rgb format");
        const int np = g.planar ? g.ch : 1;
        const bool conv = f.conv;
        v.push_back({"rgb", np, conv, g.bps, true,
                     [g, np, conv](unsigned w, unsigned h, float mul, int filter, void* const* src, const size_t* sp, void* const* dst,
                                   const size_t* dp, YuvPlane* in, YuvPlane* out) {
                         unsigned dw = 0, dh = 0;
                         YuvPlane c;
                         return srcnn::check_rgb_args(g, w, h, mul, filter, src, sp, dst, dp, conv && dst ? dst[np] : nullptr,
                                                      conv && dp ? dp[np] : 0, dw, dh, in, out, c);
                     }});
    }
    return v;
}

// Plane sizes written out, so that this section does not rest on the checkers' own row_bytes and rows.
static void check_frame_geometry()
{
    alignas(16) unsigned char buf[16];   // never read: only described
    void* p[5] = {buf, buf, buf, buf, buf};
    struct Want { size_t row_bytes; unsigned rows; };
    auto same = [](const YuvPlane& got, const Want& w) { return got.row_bytes == w.row_bytes && got.rows == w.rows && got.pitch == w.row_bytes; };
    unsigned dw, dh;
    YuvPlane in[5], out[5], conv;
    {   // I420 9x7 -> 18x14: Y 9 x 7, U / V 5 x 4; output Y 18 x 14, U / V 9 x 7.  (The planes overlap: E_ARG comes last, after
        // every plane is described.)
        srcnn::YuvGeom g;
        CHECK(srcnn::check_yuv_args(g, 9, 7, 2.f, 2, p, nullptr, p, nullptr, dw, dh, in, out) == SRCNN_E_ARG && dw == 18 && dh == 14, "I420 size");
        const Want wi[3] = {{9, 7}, {5, 4}, {5, 4}}, wo[3] = {{18, 14}, {9, 7}, {9, 7}};
        for (int k = 0; k < 3; ++k) CHECK(same(in[k], wi[k]) && same(out[k], wo[k]), "I420 plane %d", k);
    }
    {   // P010 (semi-planar 4:2:0, 16-bit words) 49x2 -> 98x4: Y 98 B x 2, UV 25 pairs = 100 B x 1; output 196 B x 4, 196 B x 2
        const srcnn_yuv_format fmt = {sizeof(srcnn_yuv_format), SRCNN_YUV_SEMIPLANAR, SRCNN_YUV_420, 10, 1};
        srcnn::YuvGeom g;
        CHECK(srcnn::yuv_geom_from_format(&fmt, g) == SRCNN_OK, "P010");
        CHECK(srcnn::check_yuv_args(g, 49, 2, 2.f, 2, p, nullptr, p, nullptr, dw, dh, in, out) == SRCNN_E_ARG, "P010 call");
        const Want wi[2] = {{98, 2}, {100, 1}}, wo[2] = {{196, 4}, {196, 2}};
        for (int k = 0; k < 2; ++k) CHECK(same(in[k], wi[k]) && same(out[k], wo[k]), "P010 plane %d", k);
    }
    {   // packed rows of 49 -> 98 pixels: YUY2 4 B per pair, Y210 8 B per pair, Y410 4 B, Y416 8 B per pixel, v210 128 B per 48
        const struct { int format; size_t in_row, out_row; } T[] = {{SRCNN_YUVP_YUY2, 100, 196}, {SRCNN_YUVP_Y210, 200, 392},
                                                                    {SRCNN_YUVP_Y410, 196, 392}, {SRCNN_YUVP_Y416, 392, 784},
                                                                    {SRCNN_YUVP_V210, 256, 384}};
        for (auto& t : T) {
            srcnn::YuvPackedGeom g;
            CHECK(srcnn::yuv_packed_geom(t.format, g) == SRCNN_OK, "packed %d", t.format);
            CHECK(srcnn::check_yuv_packed_args(g, 49, 2, 2.f, 2, buf, 0, buf, 0, dw, dh, in[0], out[0]) == SRCNN_E_ARG, "packed %d call", t.format);
            CHECK(same(in[0], Want{t.in_row, 2}) && same(out[0], Want{t.out_row, 4}), "packed %d: rows of %zu and %zu bytes", t.format,
                  in[0].row_bytes, out[0].row_bytes);
        }
    }
    {   // RGBA 12-bit interleaved 9x7 -> 18x14: 4 words per pixel = 72 B x 7 and 144 B x 14, dst_conv one word = 36 B x 14;
        // planar: 18 B x 7 and 36 B x 14 per plane
        srcnn_rgb_format fmt = {sizeof(srcnn_rgb_format), SRCNN_RGB_INTERLEAVED, SRCNN_RGB_ORDER_RGB, 1, 12};
        srcnn::RgbRule g;
        CHECK(srcnn::rgb_rule_from_format(&fmt, g) == SRCNN_OK, "rgb");
        CHECK(srcnn::check_rgb_args(g, 9, 7, 2.f, 2, p, nullptr, p, nullptr, buf, 0, dw, dh, in, out, conv) == SRCNN_E_ARG, "rgb call");
        CHECK(same(in[0], Want{72, 7}) && same(out[0], Want{144, 14}) && same(conv, Want{36, 14}), "rgba interleaved");
        fmt.layout = SRCNN_RGB_PLANAR;
        CHECK(srcnn::rgb_rule_from_format(&fmt, g) == SRCNN_OK, "rgb planar");
        CHECK(srcnn::check_rgb_args(g, 9, 7, 2.f, 2, p, nullptr, p, nullptr, nullptr, 0, dw, dh, in, out, conv) == SRCNN_E_ARG, "rgb planar call");
        for (int k = 0; k < 4; ++k) CHECK(same(in[k], Want{18, 7}) && same(out[k], Want{36, 14}), "rgba planar plane %d", k);
    }
}

static void check_frame_args()
{
    constexpr int E_ARG = SRCNN_E_ARG, E_SCALE = SRCNN_E_SCALE, E_UNS = SRCNN_E_UNSUPPORTED;
    constexpr size_t kGap = 16384;       // between plane starts of the roomy layout: far above any plane used here
    for (const Family& F : frame_families()) {
        const int np = F.np, nout = F.nout();
        // one allocation, so that a plane can be moved onto or beside another one: inputs from 8 gaps in, outputs from 16 gaps in
        std::vector<unsigned char> room(24 * kGap);
        void *src[5] = {}, *dst[5] = {};
        for (int k = 0; k < 5; ++k) { src[k] = room.data() + (8 + k) * kGap; dst[k] = room.data() + (16 + k) * kGap; }
        const size_t tight[5] = {0, 0, 0, 0, 0};

        // valid frames, tight and padded: every plane in an allocation of exactly its own size, both ends touched
        const unsigned sizes[][2] = {{1, 1}, {9, 7}, {49, 2}};
        for (auto& s : sizes)
            for (size_t pad : {(size_t)0, (size_t)64}) {
                YuvPlane in[5], out[5];
                CHECK(F.check(s[0], s[1], 2.f, 2, src, tight, dst, tight, in, out) == SRCNN_OK, "%s %ux%u roomy", F.name, s[0], s[1]);
                std::vector<std::vector<unsigned char>> mem;
                void *xs[5] = {}, *xd[5] = {};
                size_t sp[5] = {}, dp[5] = {};
                for (int k = 0; k < np; ++k) {
                    sp[k] = pad ? in[k].row_bytes + pad : 0;
                    mem.emplace_back((in[k].row_bytes + pad) * (in[k].rows - 1) + in[k].row_bytes);
                    xs[k] = mem.back().data();
                }
                for (int k = 0; k < nout; ++k) {
                    dp[k] = pad ? out[k].row_bytes + pad : 0;
                    mem.emplace_back((out[k].row_bytes + pad) * (out[k].rows - 1) + out[k].row_bytes);
                    xd[k] = mem.back().data();
                }
                YuvPlane xin[5], xout[5];
                CHECK(F.check(s[0], s[1], 2.f, 2, xs, sp, xd, dp, xin, xout) == SRCNN_OK, "%s %ux%u pad %zu", F.name, s[0], s[1], pad);
                unsigned touched = 0;
                for (int k = 0; k < np + nout; ++k) {
                    const YuvPlane& p = k < np ? xin[k] : xout[k - np];
                    CHECK(p.lo == mem[k].data() && p.hi() == mem[k].data() + mem[k].size(), "%s %ux%u pad %zu: plane %d ends %td bytes off",
                          F.name, s[0], s[1], pad, k, p.hi() - (mem[k].data() + mem[k].size()));
                    touched += p.lo[0] + p.hi()[-1];
                }
                CHECK(touched == 0, "fresh planes are zero");
            }

        // refusals, on a 9x7 frame with explicit tight pitches in the roomy layout
        YuvPlane in[5], out[5], t_in[5], t_out[5];
        CHECK(F.check(9, 7, 2.f, 2, src, tight, dst, tight, in, out) == SRCNN_OK, "%s base", F.name);
        size_t sp[5] = {}, dp[5] = {}, osize[5] = {};
        for (int k = 0; k < np; ++k) sp[k] = in[k].row_bytes;
        for (int k = 0; k < nout; ++k) { dp[k] = out[k].row_bytes; osize[k] = (size_t)(out[k].hi() - out[k].lo); }
        auto call = [&](void* const* s_, const size_t* sp_, void* const* d_, const size_t* dp_, unsigned w = 9, unsigned h = 7, float mul = 2.f,
                        int filter = 2) { return F.check(w, h, mul, filter, s_, sp_, d_, dp_, t_in, t_out); };
        CHECK(call(src, sp, dst, dp) == SRCNN_OK, "%s explicit pitches", F.name);
        for (int side = 0; side < 2; ++side)
            for (int k = 0; k < (side ? nout : np); ++k) {
                void* p2[5]; size_t q2[5];
                memcpy(p2, side ? dst : src, sizeof p2); memcpy(q2, side ? dp : sp, sizeof q2);
                q2[k] -= F.align;                                        // short pitch
                CHECK((side ? call(src, sp, dst, q2) : call(src, q2, dst, dp)) == E_ARG, "%s short pitch side %d plane %d", F.name, side, k);
                p2[k] = nullptr;
                CHECK((side ? call(src, sp, p2, dp) : call(p2, sp, dst, dp)) == (side && k == np ? SRCNN_OK : E_ARG),   // dst_conv is optional
                      "%s NULL side %d plane %d", F.name, side, k);
                if (F.align == 1) continue;
                memcpy(p2, side ? dst : src, sizeof p2); memcpy(q2, side ? dp : sp, sizeof q2);
                p2[k] = static_cast<unsigned char*>(p2[k]) + 1;          // misaligned base
                CHECK((side ? call(src, sp, p2, dp) : call(p2, sp, dst, dp)) == E_ARG, "%s odd base side %d plane %d", F.name, side, k);
                q2[k] += F.align + 1;                                    // misaligned pitch (long enough)
                CHECK((side ? call(src, sp, dst, q2) : call(src, q2, dst, dp)) == E_ARG, "%s odd pitch side %d plane %d", F.name, side, k);
            }
        // every output plane against every input plane: on its first sample, on its last, and right before / behind it
        for (int a = 0; a < np; ++a)
            for (int b = 0; b < nout; ++b) {
                unsigned char* lo = const_cast<unsigned char*>(in[a].lo);
                unsigned char* hi = const_cast<unsigned char*>(in[a].hi());
                const struct { unsigned char* at; int want; const char* what; } moves[] = {
                    {lo, E_ARG, "same start"}, {hi - F.align, E_ARG, "starts on the input's last sample"},
                    {lo - osize[b] + F.align, E_ARG, "ends on the input's first sample"}, {hi, SRCNN_OK, "starts right behind the input"},
                    {lo - osize[b], SRCNN_OK, "ends right before the input"}};
                for (auto& m : moves) {
                    void* d2[5];
                    memcpy(d2, dst, sizeof d2);
                    d2[b] = m.at;
                    CHECK(call(src, sp, d2, dp) == m.want, "%s input %d / output %d: %s", F.name, a, b, m.what);
                }
            }
        // output planes over each other: refused by the RGB call, accepted by the YUV calls
        for (int a = 0; a < nout; ++a)
            for (int b = a + 1; b < nout; ++b) {
                void* d2[5];
                memcpy(d2, dst, sizeof d2);
                d2[b] = const_cast<unsigned char*>(out[a].hi()) - F.align;
                CHECK(call(src, sp, d2, dp) == (F.out_out ? E_ARG : SRCNN_OK), "%s outputs %d and %d overlap", F.name, a, b);
                d2[b] = const_cast<unsigned char*>(out[a].hi());
                CHECK(call(src, sp, d2, dp) == SRCNN_OK, "%s outputs %d and %d adjacent", F.name, a, b);
            }
        // scale and size limits, with the codes and in the order tests/test_*_abi.py pin
        const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
        for (float mul : {0.f, -1.f, 0.1f, 0.05f, nan}) CHECK(call(src, sp, dst, dp, 9, 7, mul) == E_SCALE, "%s multiply %g", F.name, mul);
        CHECK(call(src, sp, dst, dp, 9, 7, inf) == E_UNS, "%s multiply inf", F.name);
        CHECK(call(src, sp, dst, dp, 1u << 22, 2, 4.f) == E_UNS && call(src, sp, dst, dp, 2, 1u << 20, 2.f) == E_UNS &&
              call(src, sp, dst, dp, 60000, 60000, 2.f) == E_UNS, "%s size limits", F.name);
        CHECK(call(src, sp, dst, dp, 0, 7) == E_ARG && call(src, sp, dst, dp, 9, 0) == E_ARG && call(src, sp, dst, dp, 9, 7, 2.f, 5) == E_ARG &&
              call(src, sp, dst, dp, 9, 7, 2.f, -1) == E_ARG, "%s zero size / filter", F.name);
        CHECK(call(nullptr, sp, dst, dp, 9, 7, 0.f) == E_ARG && call(src, sp, nullptr, dp, 0, 0, nan, 9) == E_ARG, "%s NULL arrays", F.name);
    }
}

// ---- the owner types (srcnn_owned.hpp) ----
static int g_live = 0, g_made = 0, g_destroyed = 0;
static std::string g_log;                 // 'd' drain, 'f' free, 'a' alloc, in call order
static bool g_alloc_fails = false;
struct TestHandleTraits { static void destroy(int* h) { ++g_destroyed; --g_live; free(h); } };
using TestHandle = srcnn::Owned<int*, TestHandleTraits>;
static int make_handle(int** out) { *out = static_cast<int*>(malloc(sizeof(int))); **out = ++g_made; ++g_live; return 0; }
struct TestAlloc {
    static void drain() { g_log += 'd'; }
    static int alloc(void** p, size_t bytes, int tag = 0)
    {
        g_log += 'a';
        if (g_alloc_fails) return -7 - tag;
        *p = malloc(bytes);
        ++g_live;
        return 0;
    }
    static void free(void* p) { g_log += 'f'; --g_live; ::free(p); }
};
using TestBuf = srcnn::GrowBuf<double, TestAlloc>;

static void check_owners()
{
    {
        TestHandle a;
        CHECK(!a && a.get() == nullptr, "a fresh owner is empty");
        a.reset();
        CHECK(make_handle(a.put()) == 0 && a && *a.get() == 1 && g_live == 1, "filled through the out-parameter");
        TestHandle b(std::move(a));
        CHECK(!a && b && *b.get() == 1 && g_destroyed == 0, "move-construct transfers, the source reads empty");
        TestHandle c;
        c = std::move(b);
        CHECK(!b && c && *c.get() == 1 && g_destroyed == 0, "move-assign transfers, the source reads empty");
        TestHandle d;
        make_handle(d.put());
        int* const old_c = c.get();
        c = std::move(d);                                      // over a full owner: handle 1 goes first, handle 2 moves in
        CHECK(g_destroyed == 1 && g_live == 1 && c.get() != old_c && *c.get() == 2 && !d, "move-assign over a full owner destroys the old handle");
        TestHandle& self = c;
        c = std::move(self);
        CHECK(c && *c.get() == 2 && g_destroyed == 1, "self-move is harmless");
        int* raw = c.release();
        CHECK(!c && raw && *raw == 2 && g_destroyed == 1 && g_live == 1, "release() hands the handle out undestroyed");
        make_handle(c.put());
        make_handle(c.put());                                  // put() on a full owner destroys what it held
        CHECK(g_destroyed == 2 && *c.get() == 4, "put() empties first");
        TestHandleTraits::destroy(raw);
        c.reset();
        c.reset();
        CHECK(g_destroyed == 4 && g_live == 0, "reset() twice is harmless");
        // a vector that reallocates moves its owners: nothing is destroyed early, everything once at the end
        std::vector<TestHandle> v;
        for (int i = 0; i < 100; ++i) { v.emplace_back(); make_handle(v.back().put()); }
        CHECK(g_destroyed == 4 && g_live == 100, "a reallocating vector destroys nothing early (%d destroyed, %d live)", g_destroyed, g_live);
        bool in_order = true;
        for (int i = 0; i < 100; ++i) in_order = in_order && *v[i].get() == 5 + i;
        CHECK(in_order, "the vector's handles are the ones created");
    }
    CHECK(g_live == 0 && g_destroyed == g_made, "every handle destroyed exactly once: %d made, %d destroyed", g_made, g_destroyed);
    {
        TestBuf b;
        CHECK(b.grow(0) == 0 && b.data() == nullptr && b.size() == 0 && g_log.empty(), "grow(0) on an empty buffer does not allocate");
        CHECK(b.grow(10) == 0 && b.size() == 10 && g_log == "a", "first growth: no drain, no free (%s)", g_log.c_str());
        double* const p = b.data();
        p[0] = 1.0; p[9] = 2.0;
        CHECK(b.grow(9) == 0 && b.grow(10) == 0 && b.data() == p && b.size() == 10 && g_log == "a", "grow-only: a smaller request keeps the block");
        g_log.clear();
        CHECK(b.grow(20) == 0 && b.size() == 20 && g_log == "dfa" && g_live == 1, "growth drains, frees, then allocates (%s)", g_log.c_str());
        b.data()[19] = 3.0;
        TestBuf c(std::move(b));
        CHECK(!b.data() && b.size() == 0 && c.size() == 20 && c.data()[19] == 3.0, "move-construct transfers");
        b = std::move(c);
        TestBuf& self = b;
        b = std::move(self);
        CHECK(!c.data() && c.size() == 0 && b.size() == 20 && b.data()[19] == 3.0 && g_live == 1, "move-assign transfers; self-move is harmless");
        CHECK(c.grow(5) == 0 && g_live == 2, "a moved-from buffer is an empty one");
        g_log.clear();
        c = std::move(b);                                      // over a full buffer: its block is freed first
        CHECK(g_log == "f" && g_live == 1 && c.size() == 20, "move-assign over a full buffer frees its block (%s)", g_log.c_str());
        g_alloc_fails = true;
        g_log.clear();
        CHECK(c.grow(40, 3) == -10 && c.data() == nullptr && c.size() == 0 && g_log == "dfa" && g_live == 0,
              "a failed allocation returns the allocator's error and leaves the buffer empty (%s)", g_log.c_str());
        CHECK(c.grow(40) == -7 && c.data() == nullptr && c.size() == 0, "and again from empty");
        g_alloc_fails = false;
        CHECK(c.grow(40) == 0 && c.size() == 40, "the next growth succeeds");
        c.data()[39] = 4.0;
        c.reset();
        c.reset();
        CHECK(c.data() == nullptr && c.size() == 0 && g_live == 0, "reset() twice is harmless");
        // emptied by assignment, as srcnn_trim empties the owners of a struct that lives on
        struct Pair { TestBuf x, y; TestHandle h[2]; } pr;
        pr.x.grow(3); pr.y.grow(4); make_handle(pr.h[1].put());
        pr = {};
        CHECK(g_live == 0 && !pr.x.data() && !pr.y.data() && !pr.h[1], "struct = {} releases every owner in it");
        std::vector<TestBuf> v;
        for (int i = 0; i < 50; ++i) { v.emplace_back(); v.back().grow(1 + i); v.back().data()[i] = i; }
        CHECK(g_live == 50, "a reallocating vector of buffers frees nothing early");
    }
    CHECK(g_live == 0, "every block freed: %d live", g_live);
}

int main()
{
    check_tables();
    check_oracle_shapes();
    check_dropin();
    check_threads();
    check_watchdog();
    check_frame_geometry();
    check_frame_args();
    check_owners();
    if (g_fail) { fprintf(stderr, "host_sanitize: %d check(s) failed\n", g_fail); return 1; }
    printf("host_sanitize: all checks passed (%d stand-in device calls)\n", g_calls.load());
    return 0;
}
