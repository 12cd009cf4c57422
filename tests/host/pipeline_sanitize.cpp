// pipeline_sanitize.cpp -- the threaded host pipeline of the product under ASan+UBSan / TSan, CPU only
// (make pipeline-asan pipeline-tsan).
//
// Links srcnn_capi.cpp, srcnn_pipeline.cpp, srcnn_comm.cpp and dropin.cpp -- unchanged -- with a fake HIP runtime
// (fake_hip.cpp: streams are worker threads, two schedules, every copy and every block checked against a registry) and the
// launchers as CPU closures (fake_kernels.cpp: footprints declared from the launchers' contracts, real resampler and colour
// arithmetic, two layer bodies), plus oracle/srcnn_oracle.c.  One scenario per process (the library reads its switches once,
// at load): `pipeline_sanitize --env <scenario>` prints the switches a scenario wants, `pipeline_sanitize <scenario>` runs it.
// The make goals run every scenario under FAKE_HIP_SCHEDULE=asap and =lazy.
//
// References: `exact` scenarios are compared byte for byte with oracle_dosrcnn / oracle_y_path; `sparse` scenarios with the
// same pixel functions run over whole planes, single-threaded, with no bands, streams or staging (oracle resampler, oracle
// colour lines).  Result buffers start as 0xFF, like every block of the fake runtime: a byte nobody wrote fails the comparison.
// Every process must end with 0 violations of the fake runtime and, after srcnn_shutdown, an empty block registry.
// Scenario `rect` runs the window route of the Y path (srcnn_y_path_rect_f32_dev: resample_window, the layers over a window,
// the store of its interior) against the crop of the frame call's result, banded and not.
//
// The three suspects of ADVICE.md:
//   suspect-a  REAL: host_is_page_locked() asked about the first byte only, so a buffer whose second half is pageable went to
//              hipMemcpy whole.  Fixed in srcnn_capi.cpp (the range's last byte is asked about too); the frame stream's
//              is_pinned() had the same shape and takes the range now.
//   suspect-b  false: SlotGuard (srcnn_capi.cpp) waits for the slot events on every way out of copy_*_any.
//   suspect-c  false: the Ctx is not published before it is complete, and its members (owner types) release the bounce slots.
// Not run: a job dropped without srcnn_process_u8_wait -- srcnn_amd.h asks for exactly one wait per begin, so a dropped job
// is a leak by contract, not a promise to check.
// TSan suppressions: none.  (The per-pixel loops of fake_kernels.cpp are not instrumented by TSan -- each closure touches its
// declared footprint from instrumented code instead -- and the TSan build links the oracle uninstrumented.)
//
// Wall time, every scenario under both schedules (the two side by side), build included, measured on 8 CPUs: make pipeline-asan
// 79 s, make pipeline-tsan 76 s; all four parameters of tests/test_host_sanitizers.py 173 s.  To get there the images were shrunk,
// not the coverage: the largest small image is 37 x 53 (the exact layers cost 7 k MAC per pixel), the stream's frames are 80 x 32
// (the narrowest whose result a 1 MB workspace limit still bands), the large image is 1008 x 700 x 3 (x2: 8.5 MB, just over the
// 8 MB at which the banded, dealt-out path begins).
//
// Teeth (each break made on a scratch copy, `lazy`): without the wait after the band stage-in copy, large-pageable and
// large-pinned fail (wrong bytes in every thread's image).  Without the wait for e_out before a stream slot is reused nothing
// fails, and nothing should: the slot's next H2D is queued on the same in-order copy stream as that D2H, and the host waits for
// that H2D before it launches the kernels that overwrite dout.  With ws.up's grow one row short nothing fails either:
// y_path_rows grows the buffer again (a drain, a free and an allocation in the middle of the call -- slower, not wrong).
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/libsrcnn_dropin.h"
#include "../../include/srcnn_amd.h"
#include "../../include/srcnn_amd_rect.h"

namespace fakehip {
unsigned long violations();
unsigned long pageable_copies();
size_t live_blocks();
size_t live_handles();
void finish();
}  // namespace fakehip
namespace fakek {
enum { kExact = 0, kSparse = 1 };
void set_layers(int body);
void layers_whole(const float* up, int W, int H, float* out, int body);
}  // namespace fakek
extern "C" {
int oracle_resample(const float* src, unsigned sw, unsigned sh, unsigned dw, unsigned dh, float* dst, int filter);
int oracle_y_path(const float* y, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, float* out, float* up, float* c1, float* c2);
int oracle_dosrcnn(const unsigned char* rgb, unsigned w, unsigned h, unsigned d, float mul, int filter, unsigned char* out, unsigned char* conv_opt);
void oracle_conv1(const float* y, unsigned w, unsigned h, float* out);
void oracle_conv2(const float* in, unsigned w, unsigned h, float* out);
void oracle_conv3(const float* in, unsigned w, unsigned h, float* out);
}

namespace {

std::atomic<int> g_failed{0};
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        if (!(cond)) {                                                         \
            ++g_failed;                                                        \
            fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                      \
            fprintf(stderr, "\n");                                             \
        }                                                                      \
    } while (0)

using Bytes = std::vector<unsigned char>;

Bytes make_image(unsigned w, unsigned h, unsigned d, unsigned seed)
{
    Bytes v((size_t)w * h * d);
    unsigned s = seed * 2654435761u + 12345u;
    for (unsigned y = 0; y < h; ++y)
        for (unsigned x = 0; x < w; ++x)
            for (unsigned c = 0; c < d; ++c) {
                s = s * 1664525u + 1013904223u;
                v[((size_t)y * w + x) * d + c] = (unsigned char)(x * 3 + y * 5 + c * 41 + ((x * y) % 23) * 7 + (s >> 27));
            }
    return v;
}
std::vector<float> make_plane(unsigned w, unsigned h, unsigned seed)
{
    std::vector<float> v((size_t)w * h);
    unsigned s = seed * 2246822519u + 7u;
    for (size_t i = 0; i < v.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        v[i] = (float)((i * 7 + (i / w) * 13) % 200) + (float)(s >> 24) * 0.125f;
    }
    return v;
}

// one doSRCNN pass as the reference does it, with the layers of `body`
void ref_dosrcnn(const unsigned char* rgb, unsigned w, unsigned h, unsigned d, float mul, int filter, int body, Bytes& out, Bytes& conv)
{
    const unsigned dw = (unsigned)((float)w * mul), dh = (unsigned)((float)h * mul);
    const size_t n = (size_t)w * h, dn = (size_t)dw * dh;
    out.assign(dn * d, 0);
    conv.assign(dn, 0);
    const bool identity = dw == w && dh == h;
    if (body == fakek::kExact && !identity) {
        CHECK(oracle_dosrcnn(rgb, w, h, d, mul, filter, out.data(), conv.data()) == 0, "oracle_dosrcnn %ux%ux%u x%g", w, h, d, mul);
        return;
    }
    // composed from the oracle's parts: the identity size (where the product copies the whole plane -- the one pinned deviation from
    // the reference's half-copied plane, DESIGN "numerics contract") and the sparse layers
    std::vector<float> pl[4], rs[4];
    for (unsigned k = 0; k < d; ++k) { pl[k].resize(n); rs[k].assign(dn, 0.f); }
    for (size_t p = 0; p < n; ++p) {
        const float r = (float)rgb[p * d + 0], g = (float)rgb[p * d + 1], b = (float)rgb[p * d + 2];
        pl[0][p] = (0.299f * r) + (0.587f * g) + (0.114f * b);
        pl[1][p] = 128.f - (0.1687f * r) - (0.3313f * g) + (0.5f * b);
        pl[2][p] = 128.f + (0.5f * r) - (0.4187f * g) - (0.0813f * b);
        if (d == 4) pl[3][p] = (float)rgb[p * d + 3];
    }
    const int cfilter = filter == 0 ? 0 : 1;
    std::vector<float> up(dn);
    for (unsigned k = 0; k < d; ++k) {
        std::vector<float>& dst = k ? rs[k] : up;
        if (identity) dst = pl[k];
        else oracle_resample(pl[k].data(), w, h, dw, dh, dst.data(), k ? cfilter : filter);
    }
    if (body == fakek::kExact) {
        std::vector<float> c1(dn * 64), c2(dn * 32);
        oracle_conv1(up.data(), dw, dh, c1.data());
        oracle_conv2(c1.data(), dw, dh, c2.data());
        oracle_conv3(c2.data(), dw, dh, rs[0].data());
    } else {
        fakek::layers_whole(up.data(), (int)dw, (int)dh, rs[0].data(), body);
    }
    for (size_t p = 0; p < dn; ++p) {
        const float fy = rs[0][p], cb = rs[1][p] - 128.f, cr = rs[2][p] - 128.f;
        float R = fy + 45.f * cr / 32.f;
        float G = fy - (11.f * cb + 23.f * cr) / 32.f;
        float B = fy + 113.f * cb / 64.f;
        R = 255.f < R ? 255.f : R; G = 255.f < G ? 255.f : G; B = 255.f < B ? 255.f : B;
        out[p * d + 0] = (unsigned char)(0.f > R ? 0.f : R);
        out[p * d + 1] = (unsigned char)(0.f > G ? 0.f : G);
        out[p * d + 2] = (unsigned char)(0.f > B ? 0.f : B);
        if (d == 4) {
            const float A = 255.f < rs[3][p] ? 255.f : rs[3][p];
            out[p * d + 3] = (unsigned char)(0.f > A ? 0.f : A);
        }
        conv[p] = (unsigned char)rs[0][p];
    }
}

void ref_y2x(const float* in, unsigned w, unsigned h, int body, std::vector<float>& out)
{
    out.assign((size_t)w * h * 4, 0.f);
    if (body == fakek::kExact) { CHECK(oracle_y_path(in, w, h, 2 * w, 2 * h, SRCNN_FILTER_BICUBIC, out.data(), nullptr, nullptr, nullptr) == 0, "oracle_y_path"); return; }
    std::vector<float> up((size_t)w * h * 4);
    oracle_resample(in, w, h, 2 * w, 2 * h, up.data(), SRCNN_FILTER_BICUBIC);
    fakek::layers_whole(up.data(), (int)(2 * w), (int)(2 * h), out.data(), body);
}

size_t first_diff(const void* a, const void* b, size_t n)
{
    const unsigned char* p = (const unsigned char*)a; const unsigned char* q = (const unsigned char*)b;
    for (size_t i = 0; i < n; ++i) if (p[i] != q[i]) return i;
    return n;
}
#define CHECK_SAME(got, want, n, ...)                                                                        \
    do {                                                                                                     \
        const size_t at_ = first_diff(got, want, n);                                                         \
        if (at_ != (n)) { CHECK(at_ == (n), __VA_ARGS__); fprintf(stderr, "    first difference at byte %zu of %zu: got %u, want %u\n", at_, (size_t)(n), ((const unsigned char*)(got))[at_], ((const unsigned char*)(want))[at_]); } \
    } while (0)

// a buffer that is either pageable (malloc) or from srcnn_host_alloc_pinned, filled with 0xFF
struct HostBuf {
    void* p = nullptr; bool pinned = false;
    HostBuf(size_t n, bool pin) : pinned(pin) { p = pin ? srcnn_host_alloc_pinned(n) : malloc(n); if (p) memset(p, 0xFF, n); }
    ~HostBuf() { if (pinned) srcnn_host_free_pinned(p); else free(p); }
    HostBuf(const HostBuf&) = delete;
    unsigned char* u8() const { return (unsigned char*)p; }
    float* f32() const { return (float*)p; }
};

// ---- 1. small images through ProcessSRCNN (exact) ----
void small_case(unsigned w, unsigned h, unsigned d, float mul, int body)
{
    const Bytes img = make_image(w, h, d, w * 31 + h * 7 + d);
    const unsigned dw = (unsigned)((float)w * mul), dh = (unsigned)((float)h * mul);
    unsigned char* out = nullptr; unsigned outsz = 0; unsigned char* conv = nullptr; unsigned convsz = 0;
    const int rc = ProcessSRCNN(img.data(), w, h, d, mul, out, outsz, &conv, &convsz);
    if (dw == 0 || dh == 0) {
        CHECK(rc == SRCNN_E_SCALE && !out && !conv, "%ux%ux%u x%g scales to nothing: rc %d", w, h, d, mul, rc);
        return;
    }
    CHECK(rc == 0, "ProcessSRCNN %ux%ux%u x%g -> %d (%s)", w, h, d, mul, rc, srcnn_last_error());
    if (rc == 0) {
        Bytes want, wconv;
        ref_dosrcnn(img.data(), w, h, d, mul, SRCNN_FILTER_BICUBIC, body, want, wconv);
        CHECK(outsz == want.size() && convsz == wconv.size(), "sizes %u / %u", outsz, convsz);
        if (outsz == want.size()) CHECK_SAME(out, want.data(), want.size(), "ProcessSRCNN %ux%ux%u x%g: image", w, h, d, mul);
        if (convsz == wconv.size()) CHECK_SAME(conv, wconv.data(), wconv.size(), "ProcessSRCNN %ux%ux%u x%g: conv", w, h, d, mul);
    }
    delete[] out;
    delete[] conv;
}
void scenario_small()
{
    fakek::set_layers(fakek::kExact);
    ConfigureFilterSRCNN(SRCNNF_Bicubic, false);
    const unsigned shapes[4][2] = {{1, 1}, {1, 17}, {13, 1}, {37, 53}};      // (37 x 53, not 67 x 131: the exact layers cost 7 k MAC per pixel)
    for (auto& s : shapes)
        for (unsigned d = 3; d <= 4; ++d)
            for (float mul : {2.0f, 1.5f, 0.75f}) small_case(s[0], s[1], d, mul, fakek::kExact);
}

// ---- 2. large banded image from 4 threads at once (sparse) ----
constexpr unsigned kLargeW = 1008, kLargeH = 700;      // x2: 2016 x 1400 x 3 = 8.47 MB >= 8 MiB, what the banded path asks for
void large_image(bool pinned, int threads)
{
    fakek::set_layers(fakek::kSparse);
    const unsigned w = kLargeW, h = kLargeH, d = 3, dw = 2 * w, dh = 2 * h;
    const Bytes img = make_image(w, h, d, 99);
    Bytes want, wconv;
    ref_dosrcnn(img.data(), w, h, d, 2.0f, SRCNN_FILTER_BICUBIC, fakek::kSparse, want, wconv);
    CHECK(srcnn_init(0) == 0, "srcnn_init: %s", srcnn_last_error());
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            HostBuf src(img.size(), pinned), out(want.size(), pinned), conv(wconv.size(), pinned);
            memcpy(src.p, img.data(), img.size());
            const int rc = srcnn_process_u8(src.u8(), w, h, d, 2.0f, SRCNN_FILTER_BICUBIC, out.u8(), conv.u8());
            CHECK(rc == 0, "thread %d: srcnn_process_u8 -> %d (%s)", t, rc, srcnn_last_error());
            CHECK_SAME(out.p, want.data(), want.size(), "thread %d: %ux%u image", t, dw, dh);
            CHECK_SAME(conv.p, wconv.data(), wconv.size(), "thread %d: %ux%u conv", t, dw, dh);
        });
    for (auto& t : th) t.join();
}

// ---- 3. asynchronous jobs, three in flight ----
void scenario_async()
{
    fakek::set_layers(fakek::kSparse);
    struct Job { unsigned w, h, d; Bytes img, want, wconv, out, conv; void* job = nullptr; };
    Job jobs[3];
    const unsigned shapes[3][3] = {{300, 200, 4}, {kLargeW, kLargeH, 3}, {211, 157, 3}};
    for (int i = 0; i < 3; ++i) {
        Job& j = jobs[i];
        j.w = shapes[i][0]; j.h = shapes[i][1]; j.d = shapes[i][2];
        j.img = make_image(j.w, j.h, j.d, 5 + i);
        ref_dosrcnn(j.img.data(), j.w, j.h, j.d, 2.0f, SRCNN_FILTER_BICUBIC, fakek::kSparse, j.want, j.wconv);
        j.out.assign(j.want.size(), 0xFF);
        j.conv.assign(j.wconv.size(), 0xFF);
    }
    for (int round = 0; round < 1; ++round) {
        for (Job& j : jobs) {
            std::fill(j.out.begin(), j.out.end(), 0xFF);
            const int rc = srcnn_process_u8_begin(j.img.data(), j.w, j.h, j.d, 2.0f, SRCNN_FILTER_BICUBIC, j.out.data(), j.conv.data(), &j.job);
            CHECK(rc == 0 && j.job, "begin -> %d (%s)", rc, srcnn_last_error());
        }
        for (Job& j : jobs) {
            const int rc = j.job ? srcnn_process_u8_wait(j.job) : -1;
            CHECK(rc == 0, "wait -> %d (%s)", rc, srcnn_last_error());
            CHECK_SAME(j.out.data(), j.want.data(), j.want.size(), "async job %ux%u round %d: image", j.w, j.h, round);
            CHECK_SAME(j.conv.data(), j.wconv.data(), j.wconv.size(), "async job %ux%u round %d: conv", j.w, j.h, round);
        }
    }
}

// ---- 4. frame stream (exact) ----
void stream_run(const char* what, bool pinned, unsigned w, unsigned h, unsigned nframes, int use_graph, const std::vector<float>& frames,
                const std::vector<float>& want)
{
    const size_t in_n = (size_t)w * h * nframes, out_n = in_n * 4;
    HostBuf in(in_n * sizeof(float), pinned), out(out_n * sizeof(float), pinned);
    memcpy(in.p, frames.data(), in_n * sizeof(float));
    const int rc = srcnn_y_upscale2x_f32_stream(in.f32(), w, h, nframes, out.f32(), use_graph);
    CHECK(rc == 0, "%s: stream %ux%u x %u, use_graph %d -> %d (%s)", what, w, h, nframes, use_graph, rc, srcnn_last_error());
    CHECK_SAME(out.p, want.data(), out_n * sizeof(float), "%s: stream %ux%u x %u, use_graph %d", what, w, h, nframes, use_graph);
}
void scenario_stream()
{
    fakek::set_layers(fakek::kExact);
    const unsigned w = 80, h = 32, nf = 6, w2 = 20, h2 = 28, nf2 = 3;      // 160 x 64 and 40 x 56 results
    std::vector<float> a, wa, b, wb, one;
    for (unsigned f = 0; f < nf; ++f) {
        const std::vector<float> p = make_plane(w, h, f + 1);
        a.insert(a.end(), p.begin(), p.end());
        ref_y2x(p.data(), w, h, fakek::kExact, one);
        wa.insert(wa.end(), one.begin(), one.end());
    }
    for (unsigned f = 0; f < nf2; ++f) {
        const std::vector<float> p = make_plane(w2, h2, f + 50);
        b.insert(b.end(), p.begin(), p.end());
        ref_y2x(p.data(), w2, h2, fakek::kExact, one);
        wb.insert(wb.end(), one.begin(), one.end());
    }
    for (int pinned = 0; pinned <= 1; ++pinned) {
        const char* kind = pinned ? "pinned" : "pageable";
        stream_run(kind, pinned != 0, w, h, 3, 0, a, wa);
        stream_run(kind, pinned != 0, w, h, nf, 2, a, wa);               // two eager frames, two captures, four replays
        // the workspace limit moves between calls: 1 MB (the least the call accepts) bands the 160-wide result (20 KB of layer-2
        // scratch per row) into passes of 47 rows, where the default limit takes its 64 rows in one
        const size_t before = srcnn_set_workspace_limit(1u << 20);
        stream_run(kind, pinned != 0, w, h, 2, 2, a, wa);
        srcnn_set_workspace_limit(before);
        if (pinned) continue;
        stream_run(kind, false, w, h, 4, 1, a, wa);
        stream_run(kind, false, w2, h2, nf2, 2, b, wb);                  // another shape on the same context: the graph is retired
        stream_run(kind, false, w, h, 2, 2, a, wa);
        srcnn_set_workspace_limit(1u << 20);
        stream_run(kind, false, w, h, 2, 0, a, wa);
        srcnn_set_workspace_limit(before);
        stream_run(kind, false, w, h, 2, 2, a, wa);
    }
}

// ---- 5. several contexts (SRCNN_DEVICES=0,0,0) ----
void scenario_multi()
{
    CHECK(srcnn_init(-1) == 0 && srcnn_context_count() == 3, "three contexts from SRCNN_DEVICES: have %d (%s)", srcnn_context_count(), srcnn_last_error());
    large_image(false, 1);                                                // dealt over three shares
    fakek::set_layers(fakek::kSparse);
    const unsigned w = 160, h = 120;
    const std::vector<float> in = make_plane(w, h, 77);
    std::vector<float> want, got((size_t)w * h * 4);
    ref_y2x(in.data(), w, h, fakek::kSparse, want);
    memset(got.data(), 0xFF, got.size() * sizeof(float));
    float* d_in = (float*)srcnn_dev_alloc(in.size() * sizeof(float));
    float* d_out = (float*)srcnn_dev_alloc(got.size() * sizeof(float));
    CHECK(d_in && d_out, "srcnn_dev_alloc");
    if (d_in && d_out) {
        CHECK(srcnn_memcpy_h2d(d_in, in.data(), in.size() * sizeof(float), nullptr) == 0, "h2d: %s", srcnn_last_error());
        for (int sub : {0, 1, 3}) {
            const int rc = srcnn_y_upscale2x_f32_node_dev(d_in, w, h, d_out, sub);
            CHECK(rc == 0, "node call, %d sub-bands -> %d (%s)", sub, rc, srcnn_last_error());
            CHECK(srcnn_memcpy_d2h(got.data(), d_out, got.size() * sizeof(float), nullptr) == 0, "d2h: %s", srcnn_last_error());
            CHECK_SAME(got.data(), want.data(), got.size() * sizeof(float), "node call, %d sub-bands", sub);
        }
    }
    srcnn_dev_free(d_in);
    srcnn_dev_free(d_out);
}

// ---- 6. lifecycle ----
void roundtrip_40mb()
{
    const size_t n = 40u << 20;
    Bytes src(n), back(n, 0xFF);
    unsigned s = 1;
    for (size_t i = 0; i < n; i += 4) { s = s * 1664525u + 1013904223u; memcpy(&src[i], &s, 4); }
    void* d = srcnn_dev_alloc(n);
    CHECK(d != nullptr, "srcnn_dev_alloc(40 MB)");
    if (!d) return;
    CHECK(srcnn_memcpy_h2d(d, src.data(), n, nullptr) == 0, "h2d 40 MB: %s", srcnn_last_error());
    CHECK(srcnn_memcpy_d2h(back.data(), d, n, nullptr) == 0, "d2h 40 MB: %s", srcnn_last_error());
    CHECK_SAME(back.data(), src.data(), n, "40 MB pageable round trip through the two bounce slots");
    srcnn_dev_free(d);
}
void scenario_lifecycle()
{
    fakek::set_layers(fakek::kSparse);
    ConfigureFilterSRCNN(SRCNNF_Bicubic, false);
    std::atomic<bool> stop{false};
    std::vector<std::thread> th;
    for (int t = 0; t < 2; ++t)
        th.emplace_back([&, t] {
            for (int i = 0; i < 6; ++i) {
                small_case(67, 131, 3 + (unsigned)t, i & 1 ? 1.5f : 2.0f, fakek::kSparse);
                small_case(13, 1, 3, 2.0f, fakek::kSparse);
            }
            stop = true;
        });
    int trims = 0;
    while (!stop.load()) { CHECK(srcnn_trim() == 0, "srcnn_trim: %s", srcnn_last_error()); ++trims; std::this_thread::yield(); }
    for (auto& t : th) t.join();
    CHECK(trims > 0, "no trim ran beside the calls");
    srcnn_shutdown();
    CHECK(fakehip::live_blocks() == 0, "%zu blocks alive after srcnn_shutdown", fakehip::live_blocks());
    CHECK(srcnn_init(0) == 0, "srcnn_init after srcnn_shutdown: %s", srcnn_last_error());
    small_case(67, 131, 4, 2.0f, fakek::kSparse);
    roundtrip_40mb();
}

// ---- 7. the three suspects ----
void scenario_suspect_a()
{
    const size_t n = 4u << 20;
    Bytes buf(n), back(n, 0xFF);
    for (size_t i = 0; i < n; ++i) buf[i] = (unsigned char)(i * 131 + (i >> 9));
    CHECK(hipHostRegister(buf.data(), n / 2, 0) == hipSuccess, "register the first half");
    void* d = srcnn_dev_alloc(n);
    CHECK(d != nullptr, "srcnn_dev_alloc");
    if (d) {
        CHECK(srcnn_memcpy_h2d(d, buf.data(), n, nullptr) == 0, "h2d: %s", srcnn_last_error());
        CHECK(fakehip::pageable_copies() == 0, "%lu pageable bytes ranges reached a HIP copy (first half registered, second pageable)", fakehip::pageable_copies());
        CHECK(srcnn_memcpy_d2h(back.data(), d, n, nullptr) == 0, "d2h: %s", srcnn_last_error());
        CHECK_SAME(back.data(), buf.data(), n, "half-registered buffer");
        // and the other way round: a result buffer whose first half only is page-locked
        std::fill(buf.begin(), buf.end(), 0xFF);
        CHECK(srcnn_memcpy_d2h(buf.data(), d, n, nullptr) == 0, "d2h into the half-registered buffer: %s", srcnn_last_error());
        CHECK(fakehip::pageable_copies() == 0, "%lu pageable ranges reached a HIP copy (D2H)", fakehip::pageable_copies());
        CHECK_SAME(buf.data(), back.data(), n, "half-registered result buffer");
    }
    srcnn_dev_free(d);
    CHECK(hipHostUnregister(buf.data()) == hipSuccess, "unregister");
}
void scenario_suspect_b()      // FAKE_HIP_FAIL=hipMemcpyAsync:3 -- the second chunk of the 40 MB copy below (the first call is srcnn_init's)
{
    const size_t n = 40u << 20;
    CHECK(srcnn_init(0) == 0, "srcnn_init: %s", srcnn_last_error());
    Bytes a(n, 0x11), b(n), back(n, 0xFF);
    for (size_t i = 0; i < n; ++i) b[i] = (unsigned char)(i * 7 + (i >> 11));
    void* da = srcnn_dev_alloc(n);
    void* db = srcnn_dev_alloc(n);
    CHECK(da && db, "srcnn_dev_alloc");
    if (da && db) {
        int rc_a = 0, rc_b = -1;
        std::thread second([&] {
            srcnn_set_context(0);
            rc_b = srcnn_memcpy_h2d(db, b.data(), n, nullptr);      // queues for the bounce slots behind the failing copy
        });
        rc_a = srcnn_memcpy_h2d(da, a.data(), n, nullptr);
        second.join();
        CHECK(rc_a != 0 || rc_b != 0, "the injected hipMemcpyAsync failure reached neither copy");
        // whichever copy took the injected failure, the other one's bytes must be whole
        void* good = rc_a == 0 ? da : db;
        const Bytes& src = rc_a == 0 ? a : b;
        CHECK(rc_a == 0 || rc_b == 0, "both copies failed: %s", srcnn_last_error());
        CHECK(srcnn_memcpy_d2h(back.data(), good, n, nullptr) == 0, "d2h: %s", srcnn_last_error());
        CHECK_SAME(back.data(), src.data(), n, "the copy beside the failed one");
    }
    srcnn_dev_free(da);
    srcnn_dev_free(db);
}
void scenario_suspect_c()      // FAKE_HIP_FAIL=hipMemcpyAsync:1 -- the fp16 weight image, after the bounce slots were page-locked
{
    const int rc = srcnn_init(0);
    CHECK(rc != 0, "the injected failure did not reach srcnn_init");
    CHECK(fakehip::live_blocks() == 0, "%zu blocks alive after a context creation that failed", fakehip::live_blocks());
    CHECK(fakehip::live_handles() == 0, "%zu streams and events alive after a context creation that failed", fakehip::live_handles());
    CHECK(srcnn_init(0) == 0, "srcnn_init after the failed one: %s", srcnn_last_error());
    fakek::set_layers(fakek::kSparse);
    small_case(13, 1, 3, 2.0f, fakek::kSparse);
}

// ---- 8. the rect route of the Y path (sparse) ----
struct RectCase { unsigned x0, y0, rw, rh; bool tight; };

// One rect of the dw x dh result into a destination of its own -- pitched, with two canary floats before and three after every
// row, or tight -- against the crop of `whole`, the result of the frame call.
void rect_case(const float* d_in, unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const RectCase& r, const std::vector<float>& whole)
{
    const size_t pitch = r.tight ? r.rw : r.rw + 5, lead = r.tight ? 0 : 2, n = pitch * r.rh + 8;
    std::vector<float> canary(n), got(n);
    for (size_t i = 0; i < n; ++i) canary[i] = -1000.f - (float)(i % 97);
    float* d_out = (float*)srcnn_dev_alloc(n * sizeof(float));
    CHECK(d_out != nullptr, "srcnn_dev_alloc");
    if (!d_out) return;
    CHECK(srcnn_memcpy_h2d(d_out, canary.data(), n * sizeof(float), nullptr) == 0, "h2d: %s", srcnn_last_error());
    const int rc = srcnn_y_path_rect_f32_dev(d_in, 0, w, h, dw, dh, filter, r.x0, r.y0, r.rw, r.rh, d_out + lead, pitch * sizeof(float), nullptr);
    CHECK(rc == 0, "rect %ux%u at (%u,%u) of %ux%u -> %d (%s)", r.rw, r.rh, r.x0, r.y0, dw, dh, rc, srcnn_last_error());
    CHECK(srcnn_memcpy_d2h(got.data(), d_out, n * sizeof(float), nullptr) == 0, "d2h: %s", srcnn_last_error());
    std::vector<float> want = canary;
    for (unsigned y = 0; y < r.rh; ++y) memcpy(&want[lead + y * pitch], &whole[(size_t)(r.y0 + y) * dw + r.x0], r.rw * sizeof(float));
    CHECK_SAME(got.data(), want.data(), n * sizeof(float), "rect %ux%u at (%u,%u) of %ux%u, filter %d: the crop of the frame, canaries untouched", r.rw, r.rh,
               r.x0, r.y0, dw, dh, filter);
    srcnn_dev_free(d_out);
}

// The frame call's result for a w x h plane (checked against the single-threaded reference), then every rect of `rects`.
void rect_plane(unsigned w, unsigned h, unsigned dw, unsigned dh, int filter, const std::vector<RectCase>& rects)
{
    const std::vector<float> in = make_plane(w, h, w + dw);
    std::vector<float> up((size_t)dw * dh), want((size_t)dw * dh), whole((size_t)dw * dh);
    oracle_resample(in.data(), w, h, dw, dh, up.data(), filter);
    fakek::layers_whole(up.data(), (int)dw, (int)dh, want.data(), fakek::kSparse);
    memset(whole.data(), 0xFF, whole.size() * sizeof(float));
    float* d_in = (float*)srcnn_dev_alloc(in.size() * sizeof(float));
    float* d_whole = (float*)srcnn_dev_alloc(whole.size() * sizeof(float));
    CHECK(d_in && d_whole, "srcnn_dev_alloc");
    if (d_in && d_whole) {
        CHECK(srcnn_memcpy_h2d(d_in, in.data(), in.size() * sizeof(float), nullptr) == 0, "h2d: %s", srcnn_last_error());
        const int rc = srcnn_y_path_f32_dev(d_in, w, h, dw, dh, filter, d_whole, nullptr);
        CHECK(rc == 0, "frame %ux%u -> %ux%u -> %d (%s)", w, h, dw, dh, rc, srcnn_last_error());
        CHECK(srcnn_memcpy_d2h(whole.data(), d_whole, whole.size() * sizeof(float), nullptr) == 0, "d2h: %s", srcnn_last_error());
        CHECK_SAME(whole.data(), want.data(), whole.size() * sizeof(float), "frame %ux%u -> %ux%u, filter %d", w, h, dw, dh, filter);
        for (const RectCase& r : rects) rect_case(d_in, w, h, dw, dh, filter, r, whole);
    }
    srcnn_dev_free(d_in);
    srcnn_dev_free(d_whole);
}

unsigned long long stage_launches(int stage)
{
    double ms = 0;
    unsigned long long n = 0;
    CHECK(srcnn_profile_read(stage, &ms, &n) == 0, "srcnn_profile_read: %s", srcnn_last_error());
    return n;
}

void scenario_rect()
{
    fakek::set_layers(fakek::kSparse);
    srcnn_profile_enable(1);      // the stage timers of the pass run too: one event pair per stage and pass
    // 37 x 53 to 74 x 106 (bicubic) and to 55 x 79 (bilinear, not an integer ratio): the four corners, an interior rect, one sample,
    // and a full-width rect with tight pitches (y_path_range's shortcut), in the same proportions on both
    const struct { unsigned dw, dh; int filter; } outs[2] = {{74, 106, SRCNN_FILTER_BICUBIC}, {55, 79, SRCNN_FILTER_BILINEAR}};
    for (const auto& o : outs) {
        const unsigned dw = o.dw, dh = o.dh, cw = 9 * dw / 74, ch = 7 * dh / 106;
        rect_plane(37, 53, dw, dh, o.filter,
                   {{0, 0, cw, ch, false}, {dw - cw, 0, cw, ch, false}, {0, dh - ch, cw, ch, false}, {dw - cw, dh - ch, cw, ch, false},
                    {23 * dw / 74, 40 * dh / 106, 20 * dw / 74, 11 * dh / 106, false}, {37 * dw / 74, 50 * dh / 106, 1, 1, false},
                    {0, 30 * dh / 106, dw, 10 * dh / 106, true}});
    }
    // one frame pass and one pass per rect, each with its three stages
    for (int st = 0; st < SRCNN_STAGE_COUNT; ++st) CHECK(stage_launches(st) == 2 * 8, "stage %d ran %llu times, not 16", st, stage_launches(st));
    // Bands.  The limit cannot go below 1 MiB, where a 74-wide window still holds all its rows: the 16-row floor of the band
    // function needs 32 * 4 * Ww * 20 bytes above 1 MiB, a window of 410 floats or more.  So a wide, flat plane of its own, 280 x 28
    // to 560 x 56 and to 420 x 42, and rects 40 rows high and at least 410 wide: three bands of 16, 16 and 8 rows, through the window
    // route (left border, right border, interior) and through y_path_range (full width, tight)
    const size_t before = srcnn_set_workspace_limit(1u << 20);
    srcnn_profile_reset();
    rect_plane(280, 28, 560, 56, SRCNN_FILTER_BICUBIC, {{0, 8, 415, 40, false}, {140, 16, 420, 40, false}, {70, 3, 430, 40, false}, {0, 9, 560, 40, true}});
    rect_plane(280, 28, 420, 42, SRCNN_FILTER_BILINEAR, {{0, 1, 412, 40, false}, {7, 2, 413, 40, false}, {0, 0, 420, 40, true}});
    // the frames: 56 rows in four bands, 42 in three; every rect in three
    for (int st = 0; st < SRCNN_STAGE_COUNT; ++st) CHECK(stage_launches(st) == 4 + 3 + 7 * 3, "stage %d ran %llu times under the 1 MiB limit, not 28", st, stage_launches(st));
    srcnn_set_workspace_limit(before);
    srcnn_profile_enable(0);
}

struct Scenario { const char* name; const char* env; std::function<void()> run; };
const std::vector<Scenario>& scenarios()
{
    static const std::vector<Scenario> all = {
        {"small", "", scenario_small},
        {"large-pageable", "", [] { large_image(false, 4); }},
        {"large-pinned", "", [] { large_image(true, 4); }},
        {"large-device-wait-in", "SRCNN_DEVICE_WAIT_IN=1", [] { large_image(false, 4); }},
        {"large-shell-unfused", "SRCNN_SHELL_UNFUSED=1", [] { large_image(false, 4); }},
        {"large-workspace-64", "SRCNN_MAX_WORKSPACE_MB=64", [] { large_image(false, 4); }},
        {"large-one-lane", "SRCNN_MAX_LANES=1", [] { large_image(false, 4); }},
        {"async-chain-0", "SRCNN_ASYNC_CHAIN=0", scenario_async},
        {"async-chain-1", "SRCNN_ASYNC_CHAIN=1", scenario_async},
        {"async-chain-2", "SRCNN_ASYNC_CHAIN=2", scenario_async},
        {"stream", "", scenario_stream},
        {"rect", "", scenario_rect},
        {"multi", "SRCNN_DEVICES=0,0,0", scenario_multi},
        {"lifecycle", "", scenario_lifecycle},
        {"suspect-a", "", scenario_suspect_a},
        {"suspect-b", "FAKE_HIP_FAIL=hipMemcpyAsync:3", scenario_suspect_b},
        {"suspect-c", "FAKE_HIP_FAIL=hipMemcpyAsync:1", scenario_suspect_c},
    };
    return all;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--list")) {
        for (const Scenario& s : scenarios()) printf("%s\n", s.name);
        return 0;
    }
    const char* name = argc >= 2 ? argv[argc - 1] : "";
    const Scenario* sc = nullptr;
    for (const Scenario& s : scenarios()) if (!strcmp(s.name, name)) sc = &s;
    if (!sc) { fprintf(stderr, "usage: %s --list | --env <scenario> | <scenario>\n", argv[0]); return 2; }
    if (argc == 3 && !strcmp(argv[1], "--env")) { printf("%s\n", sc->env); return 0; }
    if (*sc->env) {                                  // the library read its switches when it was loaded: they must be there already
        const std::string e = sc->env;
        const size_t eq = e.find('=');
        const char* have = getenv(e.substr(0, eq).c_str());
        if (!have || e.substr(eq + 1) != have) { fprintf(stderr, "scenario %s needs %s in the environment\n", name, sc->env); return 2; }
    }
    const char* sched = getenv("FAKE_HIP_SCHEDULE");
    sc->run();
    srcnn_shutdown();
    CHECK(fakehip::live_blocks() == 0, "%zu blocks of the fake runtime alive after srcnn_shutdown", fakehip::live_blocks());
    CHECK(fakehip::live_handles() == 0, "%zu streams and events alive after srcnn_shutdown", fakehip::live_handles());
    fakehip::finish();
    CHECK(fakehip::violations() == 0, "%lu violations of the HIP contract", fakehip::violations());
    if (g_failed) { fprintf(stderr, "%s [%s]: %d checks FAILED\n", name, sched ? sched : "asap", g_failed.load()); return 1; }
    printf("%s [%s]: all checks passed\n", name, sched ? sched : "asap");
    return 0;
}
