// fake_kernels.cpp -- the launchers of srcnn_kernels.h / srcnn_window.h as CPU closures on the fake HIP runtime
// (tests/host/fake_hip.cpp), for the CPU-only pipeline harness (tests/host/pipeline_sanitize.cpp).
//
// Each launcher queues ONE closure on its stream.  Before the closure touches memory it declares its footprint: every row
// range of every buffer the launcher's documented contract lets it read or write (row bases, y_rows, c2_rows, out_row0,
// out_rows, plane stride -- not what the body happens to touch), each checked against the registry of the fake runtime.  A
// range that leaves its block is a violation even where it would land in another live block, which ASan cannot see; a
// closure whose footprint is refused does not run.  The contribution tables are read from (fake) device memory, which is what
// checks the table uploads and the table cache's lifetimes.
//
// Resamplers (whole planes and the windows of the rect call) and colour shell: the real arithmetic (fp64 weight x sample, fp64 adds, one fp32 store per pass, vertical pass
// first; the split and merge lines of the reference).
// Layers: two bodies, fakek::set_layers():
//   exact   the reference's tap order and roundings with the weights of oracle_get_weights: byte for byte the oracle.
//   sparse  the same loops over a fixed subset -- per layer-2 channel the four corners and the centre of the 9x9 window, per
//           channel of layer 3 the four corners and the centre of the 5x5 window, small fixed coefficients: ~320 MAC per pixel
//           with the full 6-sample reach, so that a banded 8 MB image costs seconds under TSan.
// Both are functions of global coordinates alone (clamp-to-edge at the true frame borders only): a banded result must equal
// the whole-frame result, and a band that was handed too few halo rows is a violation.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <vector>

#include "../../libsrcnn_amd/csrc/srcnn_window.h"

#pragma clang fp contract(off)

namespace fakehip {
void violation(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
bool in_block(const void* p, size_t bytes, int kind);
void enqueue(hipStream_t s, std::function<void()> fn);
}  // namespace fakehip
extern "C" void oracle_get_weights(float* out);

namespace fakek {
enum { kExact = 0, kSparse = 1 };
void set_layers(int body);
void layers_whole(const float* up, int W, int H, float* out, int body);
}  // namespace fakek

namespace {

using fakehip::violation;

// The per-pixel loops are kept out of TSan's instrumentation (they are most of the harness's run time, and single-threaded
// arithmetic); what TSan needs to see of a closure -- that it reads and writes its footprint NOW -- Foot::range() shows it by
// touching every 256th byte of each declared range from instrumented code.  ASan and UBSan instrument everything.
#define FAKE_HOT __attribute__((no_sanitize("thread")))
std::atomic<int> g_body{fakek::kExact};

__attribute__((no_sanitize("thread"))) inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- footprints ----
struct Foot {
    const char* kernel;
    bool ok = true;
    void range(const void* p, size_t bytes, const char* what, bool write = false)
    {
        if (!bytes) return;
        if (!p || !fakehip::in_block(p, bytes, 0)) { ok = false; violation("%s: %s [%p, +%zu bytes) is not inside one live device block", kernel, what, p, bytes); return; }
        volatile unsigned char* q = static_cast<volatile unsigned char*>(const_cast<void*>(p));
        for (size_t i = 0; i < bytes; i += 256) { const unsigned char v = q[i]; if (write) q[i] = v; }
        const unsigned char v = q[bytes - 1];
        if (write) q[bytes - 1] = v;
    }
    // rows [a, b) of an axis table
    void table(const srcnn::DevAxisTable& t, int a, int b, const char* what)
    {
        if (b <= a) return;
        range(t.first + a, sizeof(int) * (size_t)(b - a), what);
        range(t.taps + a, sizeof(int) * (size_t)(b - a), what);
        range(t.weight + (size_t)a * t.stride, sizeof(double) * (size_t)(b - a) * t.stride, what);
    }
};

// source index range [lo, hi) read by destination indices [a, b), from the DEVICE copy of the table
void span_of(const srcnn::DevAxisTable& t, int a, int b, int& lo, int& hi)
{
    lo = 0x7fffffff; hi = 0;
    for (int u = a; u < b; ++u) { lo = t.first[u] < lo ? t.first[u] : lo; const int e = t.first[u] + t.taps[u]; hi = e > hi ? e : hi; }
}

// ---- resampler: one destination row, vertical pass (fp32 intermediate row) then horizontal pass ----
template <class Load>
FAKE_HOT void rs_row(Load&& load, int src_w, int y, const srcnn::DevAxisTable& tv, const srcnn::DevAxisTable& th, int dst_w, float* mid, float* out)
{
    const int s0 = tv.first[y], n = tv.taps[y];
    const double* wr = tv.weight + (size_t)y * tv.stride;
    for (int c = 0; c < src_w; ++c) {
        double acc = 0.0;
        for (int t = 0; t < n; ++t) acc = acc + wr[t] * (double)load(s0 + t, c);
        mid[c] = (float)acc;
    }
    for (int x = 0; x < dst_w; ++x) {
        const int h0 = th.first[x], hn = th.taps[x];
        const double* hw = th.weight + (size_t)x * th.stride;
        double acc = 0.0;
        for (int t = 0; t < hn; ++t) acc = acc + hw[t] * (double)mid[h0 + t];
        out[x] = (float)acc;
    }
}

FAKE_HOT inline unsigned char to_u8_sat(float v)
{
    v = (255.f < v) ? 255.f : v;
    v = (0.f > v) ? 0.f : v;
    return (unsigned char)v;
}

// what the real k_rs2d family accepts: an up-scale in both axes with short monotone tables whose tile spans fit its LDS rows
bool rs2d_shape_ok(int src_w, int src_h, int dst_w, int dst_h, const srcnn::DevAxisTable& tv, const srcnn::DevAxisTable& th)
{
    if (dst_w < src_w || dst_h < src_h || dst_w <= 0 || dst_h <= 0) return false;
    if (!tv.monotone || !th.monotone || !tv.h_first || !th.h_first || !tv.h_taps || !th.h_taps) return false;
    if (tv.max_taps > 8 || th.max_taps > 8) return false;
    for (int x0 = 0; x0 < dst_w; x0 += 256) {
        const int xl = (x0 + 256 < dst_w ? x0 + 256 : dst_w) - 1;
        if (th.h_first[xl] + th.h_taps[xl] - th.h_first[x0] + 1 > 272) return false;
    }
    return true;
}

// ---- layers ----
const float* weights()
{
    static float w[srcnn::kWeightCount];
    static std::once_flag once;
    std::call_once(once, [] { oracle_get_weights(w); });
    return w;
}
constexpr int OFF_B1 = 0, OFF_W1 = 64, OFF_B2 = OFF_W1 + 64 * 81, OFF_W2 = OFF_B2 + 32, OFF_B3 = OFF_W2 + 32 * 64, OFF_W3 = OFF_B3 + 1;

// the fixed coefficients of the sparse bodies: the centre tap carries the signal (0.5 into layer 2, 1/32 per channel out of it),
// the corners small signed weights, so that the result stays inside (0, 255) and depends on every one of the 6 + 6 halo samples
struct SparseCoef {
    float c12[32][5], c3[32][5];
    SparseCoef()
    {
        for (int m = 0; m < 32; ++m)
            for (int t = 0; t < 5; ++t) {
                c12[m][t] = t == 2 ? 0.5f : (float)((m + t) % 3 - 1) * 0.0625f;
                c3[m][t] = t == 2 ? 0.03125f : (float)((m * 3 + t) % 5 - 2) * 0.0009765625f;
            }
    }
};
const SparseCoef g_sparse;
const float (&kSparse12)[32][5] = g_sparse.c12;
const float (&kSparse3)[32][5] = g_sparse.c3;

// layers 1+2 of one pixel; rows[i] = row clamp(y + i - 4) of the upscaled plane
FAKE_HOT void conv12_pixel_exact(const float* const rows[9], int W, int x, float* c2 /*[32]*/)
{
    const float* wt = weights();
    float v[81];
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) v[i * 9 + j] = rows[i][clampi(x + j - 4, 0, W - 1)];
    float c1[64];
    for (int k = 0; k < 64; ++k) {
        const float* ker = wt + OFF_W1 + k * 81;
        float acc = 0;
        for (int t = 0; t < 81; ++t) acc += ker[t] * v[t];
        acc += wt[OFF_B1 + k];
        c1[k] = (acc >= 0) ? acc : 0;
    }
    for (int m = 0; m < 32; ++m) {
        const float* ker = wt + OFF_W2 + m * 64;
        float acc = 0;
        for (int f = 0; f < 64; ++f) acc += c1[f] * ker[f];
        acc += wt[OFF_B2 + m];
        c2[m] = (acc >= 0) ? acc : 0;
    }
}
FAKE_HOT void conv12_pixel_sparse(const float* const rows[9], int W, int x, float* c2)
{
    const int xl = clampi(x - 4, 0, W - 1), xr = clampi(x + 4, 0, W - 1);
    const float v[5] = {rows[0][xl], rows[0][xr], rows[4][x], rows[8][xl], rows[8][xr]};
    for (int m = 0; m < 32; ++m) {
        float acc = 0;
        for (int t = 0; t < 5; ++t) acc += kSparse12[m][t] * v[t];
        acc += 0.125f * (float)(m % 4);
        c2[m] = (acc >= 0) ? acc : 0;
    }
}
// layer 3 of one pixel; rows[dy] = row clamp(y + dy - 2) of layer-2 plane 0, plane m is `plane` floats further
FAKE_HOT float conv3_pixel_exact(const float* const rows[5], size_t plane, int W, int x)
{
    const float* wt = weights();
    int gx[5];
    for (int dx = 0; dx < 5; ++dx) gx[dx] = clampi(x + dx - 2, 0, W - 1);
    float sum = 0;
    for (int m = 0; m < 32; ++m) {
        double acc = 0;
        for (int dy = 0; dy < 5; ++dy)
            for (int dx = 0; dx < 5; ++dx) acc += wt[OFF_W3 + m * 25 + dx * 5 + dy] * rows[dy][m * plane + gx[dx]];
        sum += acc;
    }
    sum += wt[OFF_B3];
    sum = sum > 0.f ? sum : 0.f;
    sum = sum < 255.f ? sum : 255.f;
    return sum;
}
FAKE_HOT float conv3_pixel_sparse(const float* const rows[5], size_t plane, int W, int x)
{
    const int xl = clampi(x - 2, 0, W - 1), xr = clampi(x + 2, 0, W - 1);
    float sum = 0;
    for (int m = 0; m < 32; ++m) {
        const float v[5] = {rows[0][m * plane + xl], rows[0][m * plane + xr], rows[2][m * plane + x], rows[4][m * plane + xl], rows[4][m * plane + xr]};
        double acc = 0;
        for (int t = 0; t < 5; ++t) acc += kSparse3[m][t] * v[t];
        sum += acc;
    }
    sum += 0.5f;
    sum = sum > 0.f ? sum : 0.f;
    sum = sum < 255.f ? sum : 255.f;
    return sum;
}

// layers 1+2 for output rows [row0, row0 + rows): Y holds rows [y_base, y_base + y_rows), C2 row row0 at offset 0 of each plane
FAKE_HOT void conv12_rows(const char* who, int body, const float* Y, int W, int H, int y_base, int y_rows, float* C2, size_t plane, int row0, int rows)
{
    bool short_halo = false;
    float c2[32];
    for (int y = row0; y < row0 + rows; ++y) {
        const float* r[9];
        for (int i = 0; i < 9; ++i) {
            int gy = clampi(y + i - 4, 0, H - 1);
            if (gy < y_base || gy >= y_base + y_rows) { short_halo = true; gy = clampi(gy, y_base, y_base + y_rows - 1); }
            r[i] = Y + (size_t)(gy - y_base) * W;
        }
        for (int x = 0; x < W; ++x) {
            if (body == fakek::kExact) conv12_pixel_exact(r, W, x, c2);
            else conv12_pixel_sparse(r, W, x, c2);
            for (int m = 0; m < 32; ++m) C2[m * plane + (size_t)(y - row0) * W + x] = c2[m];
        }
    }
    if (short_halo) violation("%s: output rows [%d, +%d) of a %d-row frame need rows outside the [%d, +%d) it was handed", who, row0, rows, H, y_base, y_rows);
}
FAKE_HOT void conv3_rows(const char* who, int body, const float* C2, size_t plane, int W, int H, int c2_base, int c2_rows, float* out, int row0, int rows)
{
    bool short_halo = false;
    for (int y = row0; y < row0 + rows; ++y) {
        const float* r[5];
        for (int dy = 0; dy < 5; ++dy) {
            int gy = clampi(y + dy - 2, 0, H - 1);
            if (gy < c2_base || gy >= c2_base + c2_rows) { short_halo = true; gy = clampi(gy, c2_base, c2_base + c2_rows - 1); }
            r[dy] = C2 + (size_t)(gy - c2_base) * W;
        }
        float* o = out + (size_t)(y - row0) * W;
        for (int x = 0; x < W; ++x) o[x] = body == fakek::kExact ? conv3_pixel_exact(r, plane, W, x) : conv3_pixel_sparse(r, plane, W, x);
    }
    if (short_halo) violation("%s: output rows [%d, +%d) of a %d-row frame need layer-2 rows outside the [%d, +%d) it was handed", who, row0, rows, H, c2_base, c2_rows);
}

void not_modelled(const char* what) { violation("%s is not modelled by the fake kernels (no scenario of the harness may reach it)", what); }

}  // namespace

namespace fakek {

void set_layers(int body) { g_body = body; }

// The three layers over a whole plane, single-threaded, no bands, no streams: the reference of the sparse scenarios.
// (Strips of 32 rows keep the 32 layer-2 planes of an 8 MB image out of memory; the pixels are functions of global coordinates.)
void layers_whole(const float* up, int W, int H, float* out, int body)
{
    const int strip = 32;
    std::vector<float> c2((size_t)32 * W * (strip + 4));
    for (int a = 0; a < H; a += strip) {
        const int b = a + strip < H ? a + strip : H;
        const int ca = a >= 2 ? a - 2 : 0, cb = b + 2 < H ? b + 2 : H;
        const size_t plane = (size_t)W * (cb - ca);
        conv12_rows("reference", body, up, W, H, 0, H, c2.data(), plane, ca, cb - ca);
        conv3_rows("reference", body, c2.data(), plane, W, H, ca, cb - ca, out + (size_t)a * W, a, b - a);
    }
}

}  // namespace fakek

namespace srcnn {

hipError_t upload_weights(const DevWeights&) { return hipSuccess; }
hipError_t fused_f16_prepare() { return hipSuccess; }
hipError_t rs2d_prepare() { return hipSuccess; }
hipError_t conv12_mfma_prepare() { return hipSuccess; }
void conv12_grid_info(int num_cus, int* blocks, int* tile_rows)
{
    if (blocks) *blocks = kConv12BlocksPerCU * num_cus;
    if (tile_rows) *tile_rows = kConv12TileRows;
}

void launch_resample_cols(const float* src, int w, int src_row_base, float* dst, int dst_row0, int dst_rows, const DevAxisTable& t, hipStream_t s)
{
    if (dst_rows <= 0) return;
    fakehip::enqueue(s, [=] {
        Foot f{"resample_cols"};
        f.table(t, dst_row0, dst_row0 + dst_rows, "table rows");
        if (!f.ok) return;
        int lo, hi;
        span_of(t, dst_row0, dst_row0 + dst_rows, lo, hi);
        if (lo < src_row_base) { violation("resample_cols: rows [%d, +%d) read source row %d below the base %d", dst_row0, dst_rows, lo, src_row_base); return; }
        f.range(src + (size_t)(lo - src_row_base) * w, sizeof(float) * (size_t)(hi - lo) * w, "source rows");
        f.range(dst, sizeof(float) * (size_t)dst_rows * w, "destination rows", true);
        if (!f.ok) return;
        for (int ry = 0; ry < dst_rows; ++ry) {
            const int y = dst_row0 + ry, s0 = t.first[y], n = t.taps[y];
            const double* wr = t.weight + (size_t)y * t.stride;
            for (int x = 0; x < w; ++x) {
                double acc = 0.0;
                for (int k = 0; k < n; ++k) acc = acc + wr[k] * (double)src[(size_t)(s0 + k - src_row_base) * w + x];
                dst[(size_t)ry * w + x] = (float)acc;
            }
        }
    });
}

void launch_resample_rows(const float* src, int src_w, float* dst, int dst_w, int rows, const DevAxisTable& t, hipStream_t s)
{
    if (rows <= 0) return;
    fakehip::enqueue(s, [=] {
        Foot f{"resample_rows"};
        f.table(t, 0, dst_w, "table rows");
        f.range(src, sizeof(float) * (size_t)rows * src_w, "source rows");
        f.range(dst, sizeof(float) * (size_t)rows * dst_w, "destination rows", true);
        if (!f.ok) return;
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < dst_w; ++x) {
                const float* in = src + (size_t)y * src_w + t.first[x];
                const double* wr = t.weight + (size_t)x * t.stride;
                double acc = 0.0;
                for (int k = 0; k < t.taps[x]; ++k) acc = acc + wr[k] * (double)in[k];
                dst[(size_t)y * dst_w + x] = (float)acc;
            }
    });
}

bool rs2d_fits(int, int src_w, int src_h, int dst_w, int dst_h, int r0, int r1, const DevAxisTable& tv, const DevAxisTable& th)
{
    return r1 > r0 && rs2d_shape_ok(src_w, src_h, dst_w, dst_h, tv, th);
}

bool launch_rs2d(const YSource& src, int src_w, int src_h, float* dst, int dst_w, int dst_h, int dst_row0, int dst_rows,
                 const DevAxisTable& tv, const DevAxisTable& th, hipStream_t s)
{
    if (!src.plane && !(src.rgb && (src.depth == 3 || src.depth == 4))) return false;
    if (dst_rows <= 0 || !rs2d_shape_ok(src_w, src_h, dst_w, dst_h, tv, th)) return false;
    fakehip::enqueue(s, [=] {
        Foot f{"rs2d"};
        f.table(tv, dst_row0, dst_row0 + dst_rows, "vertical table rows");
        f.table(th, 0, dst_w, "horizontal table rows");
        if (!f.ok) return;
        int lo, hi;
        span_of(tv, dst_row0, dst_row0 + dst_rows, lo, hi);
        if (hi > src_h) { violation("rs2d: rows [%d, +%d) read source row %d of %d", dst_row0, dst_rows, hi - 1, src_h); return; }
        if (src.plane) f.range(src.plane + (size_t)lo * src_w, sizeof(float) * (size_t)(hi - lo) * src_w, "source rows");
        else f.range(src.rgb + (size_t)lo * src_w * src.depth, (size_t)(hi - lo) * src_w * src.depth, "source image rows");
        f.range(dst, sizeof(float) * (size_t)dst_rows * dst_w, "destination rows", true);
        if (!f.ok) return;
        std::vector<float> mid((size_t)src_w);
        const int d = src.depth;
        for (int ry = 0; ry < dst_rows; ++ry) {
            float* out = dst + (size_t)ry * dst_w;
            if (src.plane) rs_row([&](int r, int c) FAKE_HOT { return src.plane[(size_t)r * src_w + c]; }, src_w, dst_row0 + ry, tv, th, dst_w, mid.data(), out);
            else rs_row([&](int r, int c) FAKE_HOT {
                     const unsigned char* q = src.rgb + ((size_t)r * src_w + c) * d;
                     const float R = (float)q[0], G = (float)q[1], B = (float)q[2];
                     return (0.299f * R) + (0.587f * G) + (0.114f * B);
                 }, src_w, dst_row0 + ry, tv, th, dst_w, mid.data(), out);
        }
    });
    return true;
}

bool launch_merge_fused(const unsigned char* rgb_src, int src_w, int src_h, int depth, const float* Yp, unsigned char* rgb_out,
                        unsigned char* conv_opt, int dst_w, int dst_h, int dst_row0, int dst_rows, const DevAxisTable& tv,
                        const DevAxisTable& th, hipStream_t s)
{
    if ((depth != 3 && depth != 4) || dst_rows <= 0 || !rs2d_shape_ok(src_w, src_h, dst_w, dst_h, tv, th)) return false;
    fakehip::enqueue(s, [=] {
        Foot f{"merge_fused"};
        f.table(tv, dst_row0, dst_row0 + dst_rows, "vertical table rows");
        f.table(th, 0, dst_w, "horizontal table rows");
        if (!f.ok) return;
        int lo, hi;
        span_of(tv, dst_row0, dst_row0 + dst_rows, lo, hi);
        if (hi > src_h) { violation("merge_fused: rows [%d, +%d) read source row %d of %d", dst_row0, dst_rows, hi - 1, src_h); return; }
        const size_t pn = (size_t)dst_rows * dst_w;
        f.range(rgb_src + (size_t)lo * src_w * depth, (size_t)(hi - lo) * src_w * depth, "source image rows");
        f.range(Yp, sizeof(float) * pn, "Y' rows");
        f.range(rgb_out, pn * depth, "result rows", true);
        if (conv_opt) f.range(conv_opt, pn, "truncated Y' rows", true);
        if (!f.ok) return;
        std::vector<float> mid((size_t)src_w), pl[3];
        for (auto& p : pl) p.resize((size_t)dst_w);
        for (int ry = 0; ry < dst_rows; ++ry) {
            const int y = dst_row0 + ry;
            for (int k = 0; k < depth - 1; ++k)
                rs_row([&](int r, int c) FAKE_HOT {
                    const unsigned char* q = rgb_src + ((size_t)r * src_w + c) * depth;
                    const float R = (float)q[0], G = (float)q[1], B = (float)q[2];
                    if (k == 0) return 128.f - (0.1687f * R) - (0.3313f * G) + (0.5f * B);
                    if (k == 1) return 128.f + (0.5f * R) - (0.4187f * G) - (0.0813f * B);
                    return (float)q[3];
                }, src_w, y, tv, th, dst_w, mid.data(), pl[k].data());
            for (int x = 0; x < dst_w; ++x) {
                const size_t p = (size_t)ry * dst_w + x;
                const float fy = Yp[p], cb = pl[0][x] - 128.f, cr = pl[1][x] - 128.f;
                rgb_out[p * depth + 0] = to_u8_sat(fy + 45.f * cr / 32.f);
                rgb_out[p * depth + 1] = to_u8_sat(fy - (11.f * cb + 23.f * cr) / 32.f);
                rgb_out[p * depth + 2] = to_u8_sat(fy + 113.f * cb / 64.f);
                if (depth == 4) rgb_out[p * depth + 3] = to_u8_sat(pl[2][x]);
                if (conv_opt) conv_opt[p] = (unsigned char)fy;
            }
        }
    });
    return true;
}

void launch_rgb_split(const unsigned char* rgb, size_t n, int d, float* Yp, float* Cb, float* Cr, float* A, hipStream_t s)
{
    if (!n) return;
    fakehip::enqueue(s, [=] {
        Foot f{"rgb_split"};
        f.range(rgb, n * d, "image");
        f.range(Yp, sizeof(float) * n, "Y plane", true);
        f.range(Cb, sizeof(float) * n, "Cb plane", true);
        f.range(Cr, sizeof(float) * n, "Cr plane", true);
        if (d == 4) f.range(A, sizeof(float) * n, "A plane", true);
        if (!f.ok) return;
        for (size_t p = 0; p < n; ++p) {
            const float r = (float)rgb[p * d + 0], g = (float)rgb[p * d + 1], b = (float)rgb[p * d + 2];
            Yp[p] = (0.299f * r) + (0.587f * g) + (0.114f * b);
            Cb[p] = 128.f - (0.1687f * r) - (0.3313f * g) + (0.5f * b);
            Cr[p] = 128.f + (0.5f * r) - (0.4187f * g) - (0.0813f * b);
            if (d == 4) A[p] = (float)rgb[p * d + 3];
        }
    });
}

void launch_ycc_merge(const float* Yp, const float* Cb, const float* Cr, const float* A, size_t n, int d, unsigned char* rgb,
                      unsigned char* conv_opt, hipStream_t s)
{
    if (!n) return;
    fakehip::enqueue(s, [=] {
        Foot f{"ycc_merge"};
        f.range(Yp, sizeof(float) * n, "Y' plane");
        f.range(Cb, sizeof(float) * n, "Cb' plane");
        f.range(Cr, sizeof(float) * n, "Cr' plane");
        if (d == 4) f.range(A, sizeof(float) * n, "A' plane");
        f.range(rgb, n * d, "result", true);
        if (conv_opt) f.range(conv_opt, n, "truncated Y'", true);
        if (!f.ok) return;
        for (size_t p = 0; p < n; ++p) {
            const float fy = Yp[p], cb = Cb[p] - 128.f, cr = Cr[p] - 128.f;
            rgb[p * d + 0] = to_u8_sat(fy + 45.f * cr / 32.f);
            rgb[p * d + 1] = to_u8_sat(fy - (11.f * cb + 23.f * cr) / 32.f);
            rgb[p * d + 2] = to_u8_sat(fy + 113.f * cb / 64.f);
            if (d == 4) rgb[p * d + 3] = to_u8_sat(A[p]);
            if (conv_opt) conv_opt[p] = (unsigned char)fy;
        }
    });
}

void launch_conv12_mfma(const float* Y, int W, int H, int y_row_base, int y_rows, float* C2, size_t plane_stride, int out_row0,
                        int out_rows, int relax, bool, int, hipStream_t s, unsigned long long* clk, unsigned* queue)
{
    // (tiers: that instance reads and writes what the other strict ones do and computes the same bits, so one closure serves both)
    if (out_rows <= 0) return;
    if (relax) { not_modelled("a non-parity tier of layers 1+2"); return; }
    const int body = g_body.load();
    fakehip::enqueue(s, [=] {
        Foot f{"conv12"};
        f.range(Y, sizeof(float) * (size_t)y_rows * W, "upscaled Y rows");
        if ((size_t)out_rows * W > plane_stride) { violation("conv12: %d rows of %d do not fit the plane stride %zu", out_rows, W, plane_stride); return; }
        f.range(C2, sizeof(float) * ((size_t)(C2N - 1) * plane_stride + (size_t)out_rows * W), "layer-2 planes", true);
        if (queue) f.range(queue, 2 * sizeof(unsigned), "tile queue", true);
        if (clk) f.range(clk, 2 * sizeof(unsigned long long), "clock probe slot", true);
        if (!f.ok) return;
        if (queue && (queue[0] | queue[1])) violation("conv12: the tile queue is not zero at launch (%u, %u)", queue[0], queue[1]);
        conv12_rows("conv12", body, Y, W, H, y_row_base, y_rows, C2, plane_stride, out_row0, out_rows);
    });
}

void launch_conv3(const float* C2, size_t plane_stride, int W, int H, int c2_row_base, int c2_rows, float* out, int out_row0,
                  int out_rows, int relax, hipStream_t s)
{
    if (out_rows <= 0) return;
    if (relax & (RELAX_L3_X64 | RELAX_L3_F32)) { not_modelled("a non-parity tier of layer 3"); return; }
    const int body = g_body.load();
    fakehip::enqueue(s, [=] {
        Foot f{"conv3"};
        if ((size_t)c2_rows * W > plane_stride) { violation("conv3: %d rows of %d do not fit the plane stride %zu", c2_rows, W, plane_stride); return; }
        f.range(C2, sizeof(float) * ((size_t)(C2N - 1) * plane_stride + (size_t)c2_rows * W), "layer-2 planes");
        f.range(out, sizeof(float) * (size_t)out_rows * W, "result rows", true);
        if (!f.ok) return;
        conv3_rows("conv3", body, C2, plane_stride, W, H, c2_row_base, c2_rows, out, out_row0, out_rows);
    });
}

// ---- the window kernels of the rect call (srcnn_window.h): the arithmetic of the two passes above, over a window ----

// A strided block of w x rows floats is declared row by row: the floats between two rows belong to the caller (the canary columns
// of a pitched destination) or to nobody (past the end of a window of the source), and the contract touches none of them.
static void strided(Foot& f, const float* p, size_t stride, int w, int rows, const char* what, bool write = false)
{
    if (stride == (size_t)w) { f.range(p, sizeof(float) * (size_t)rows * w, what, write); return; }
    for (int y = 0; y < rows && f.ok; ++y) f.range(p + (size_t)y * stride, sizeof(float) * (size_t)w, what, write);
}

void launch_window_rows(const float* src, size_t src_stride, int src_col_base, float* dst, int c0, int nc, int rows, const DevAxisTable& t, hipStream_t s)
{
    if (nc <= 0 || rows <= 0) return;
    fakehip::enqueue(s, [=] {
        Foot f{"window_rows"};
        f.table(t, c0, c0 + nc, "table rows");
        if (!f.ok) return;
        int lo, hi;
        span_of(t, c0, c0 + nc, lo, hi);
        if (lo < src_col_base) { violation("window_rows: columns [%d, +%d) read source column %d below the base %d", c0, nc, lo, src_col_base); return; }
        strided(f, src + (lo - src_col_base), src_stride, hi - lo, rows, "source columns");
        f.range(dst, sizeof(float) * (size_t)rows * nc, "destination window", true);
        if (!f.ok) return;
        for (int y = 0; y < rows; ++y)
            for (int xi = 0; xi < nc; ++xi) {
                const int x = c0 + xi;
                const float* in = src + (size_t)y * src_stride + (t.first[x] - src_col_base);
                const double* wr = t.weight + (size_t)x * t.stride;
                double acc = 0.0;
                for (int k = 0; k < t.taps[x]; ++k) acc = acc + wr[k] * (double)in[k];
                dst[(size_t)y * nc + xi] = (float)acc;
            }
    });
}

void launch_window_cols(const float* src, size_t src_stride, int src_row_base, float* dst, int nc, int r0, int rows, const DevAxisTable& t, hipStream_t s)
{
    if (nc <= 0 || rows <= 0) return;
    fakehip::enqueue(s, [=] {
        Foot f{"window_cols"};
        f.table(t, r0, r0 + rows, "table rows");
        if (!f.ok) return;
        int lo, hi;
        span_of(t, r0, r0 + rows, lo, hi);
        if (lo < src_row_base) { violation("window_cols: rows [%d, +%d) read source row %d below the base %d", r0, rows, lo, src_row_base); return; }
        strided(f, src + (size_t)(lo - src_row_base) * src_stride, src_stride, nc, hi - lo, "source rows");
        f.range(dst, sizeof(float) * (size_t)rows * nc, "destination window", true);
        if (!f.ok) return;
        for (int ry = 0; ry < rows; ++ry) {
            const int y = r0 + ry, s0 = t.first[y] - src_row_base, n = t.taps[y];
            const double* wr = t.weight + (size_t)y * t.stride;
            for (int xi = 0; xi < nc; ++xi) {
                double acc = 0.0;
                for (int k = 0; k < n; ++k) acc = acc + wr[k] * (double)src[(size_t)(s0 + k) * src_stride + xi];
                dst[(size_t)ry * nc + xi] = (float)acc;
            }
        }
    });
}

void launch_window_copy(const float* src, size_t src_stride, float* dst, size_t dst_stride, int w, int rows, hipStream_t s)
{
    if (w <= 0 || rows <= 0) return;
    fakehip::enqueue(s, [=] {
        Foot f{"window_copy"};
        strided(f, src, src_stride, w, rows, "source window");
        strided(f, dst, dst_stride, w, rows, "destination rows", true);
        if (!f.ok) return;
        for (int y = 0; y < rows; ++y) memcpy(dst + (size_t)y * dst_stride, src + (size_t)y * src_stride, sizeof(float) * (size_t)w);
    });
}

// reached by no scenario of the harness (strict tier, no stage-level call): defined for the link, loud if ever run
void launch_fused_f16(const float*, int, int, int, int, float*, int, int, const FusedF16Weights*, int, hipStream_t, unsigned long long*) { not_modelled("launch_fused_f16"); }
void launch_conv1_planes(const float*, int, int, float*, hipStream_t) { not_modelled("launch_conv1_planes"); }
void launch_conv2_planes(const float*, size_t, float*, hipStream_t) { not_modelled("launch_conv2_planes"); }

}  // namespace srcnn
