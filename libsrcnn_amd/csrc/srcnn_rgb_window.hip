// srcnn_rgb_window.hip -- the colour shell of the RGB(A) rect call (include/srcnn_amd_rgb_rect.h) over a WINDOW of the image:
// what srcnn_rgb.hip does for whole rows of whole planes, at the cost of the rect.
//
//   k_rgb_window_y       a rectangle of the integer source plane(s) -> a tight float32 Y window (the source of the window Y
//                        path, y_path_rect): the read rules and the Y line of k_rgb_unpack, nothing else stored -- the Y path
//                        needs the 6-sample halo, chroma does not
//   k_rgb_window_merge   one launch per band: Cb', Cr' (and A') of a 64 x 16 tile of the rect resampled straight from the
//                        integer source, merged with the finished Y' rows and written in the caller's format (and the
//                        truncated Y' plane): split of k_rgb_unpack -> the tile resampler (srcnn_window_tile.h, which describes
//                        its four steps and says which shapes it serves) -> merge and to_code of k_rgb_pack, with that kernel's
//                        vector / scalar stores
//
// The pixel rules are srcnn_colour_rules.h, shared with srcnn_rgb.hip.  A thread stores only pixels of its tile that lie inside
// the rect.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_rgb.h"
#include "srcnn_window_tile.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr unsigned kChunk = kTileChunk;          // pixels per thread, of both kernels

struct WinY {
    const unsigned char* p[4];                   // integer planes at the window's first sample (interleaved: p[0] only)
    size_t pitch[4];
    float* y;                                    // tight, w floats per row
    unsigned w, rows;                            // the window
    unsigned mask;
    float down;
    int bgr, int_vec, flt_vec;
};

struct WinMerge {
    const unsigned char* sp[4];                  // the WHOLE source planes
    size_t spitch[4];
    unsigned char* dp[4];                        // destination planes: pixel (x0, y0) of the rect first
    size_t dpitch[4];
    unsigned char* conv;                         // truncated Y', or NULL
    size_t conv_pitch;
    const float* y;                              // Y' of the band: tight, rw floats per row
    unsigned x0, gy0;                            // output column of the rect's first column, output row of the band's first row
    unsigned row0;                               // row of the rect at which the band starts
    unsigned rw, rows;                           // columns of the rect, rows of the band
    unsigned w, h;                               // source size
    TileTables t;                                // horizontal table (dw <- w), vertical table (dh <- h)
    unsigned mask;
    float down, up;
    int bgr, int_vec, conv_vec;
};

template <int BPS, bool PLANAR, int D>
__global__ __launch_bounds__(256) void k_rgb_window_y(const WinY a)
{
    const unsigned cpr = (a.w + kChunk - 1) / kChunk;
    const unsigned total = cpr * a.rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * kChunk;
        const unsigned n = min(kChunk, a.w - c);
        unsigned v[kChunk][3];                   // [pixel][channel in memory order]; alpha is not read
        if (n == kChunk && a.int_vec) {
            if constexpr (PLANAR) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const unsigned* q = reinterpret_cast<const unsigned*>(a.p[k] + (size_t)r * a.pitch[k] + (size_t)c * BPS);
                    unsigned wd[BPS];
#pragma unroll
                    for (int t = 0; t < BPS; ++t) wd[t] = q[t];
#pragma unroll
                    for (int px = 0; px < (int)kChunk; ++px) v[px][k] = sample_of<BPS>(wd, px);
                }
            } else {
                const unsigned* q = reinterpret_cast<const unsigned*>(a.p[0] + (size_t)r * a.pitch[0] + (size_t)c * D * BPS);
                unsigned wd[D * BPS];
#pragma unroll
                for (int t = 0; t < D * BPS; ++t) wd[t] = q[t];
#pragma unroll
                for (int px = 0; px < (int)kChunk; ++px)
#pragma unroll
                    for (int k = 0; k < 3; ++k) v[px][k] = sample_of<BPS>(wd, px * D + k);
            }
        } else {
#pragma unroll
            for (int px = 0; px < (int)kChunk; ++px)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    v[px][k] = 0;
                    if ((unsigned)px < n) {
                        const unsigned char* q = PLANAR ? a.p[k] + (size_t)r * a.pitch[k] + (size_t)(c + px) * BPS
                                                        : a.p[0] + (size_t)r * a.pitch[0] + ((size_t)(c + px) * D + k) * BPS;
                        v[px][k] = load_scalar<BPS>(q);
                    }
                }
        }
        float yv[kChunk];
#pragma unroll
        for (int px = 0; px < (int)kChunk; ++px) {
            float ch[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) ch[k] = (float)(v[px][k] & a.mask) * a.down;
            const float r_ = a.bgr ? ch[2] : ch[0], g = ch[1], b = a.bgr ? ch[0] : ch[2];
            yv[px] = split_y(r_, g, b);
        }
        store_floats<kChunk>(a.y + (size_t)r * a.w + c, yv, n, a.flt_vec);
    }
}

template <int BPS, bool PLANAR, int D>
__global__ __launch_bounds__(256) void k_rgb_window_merge(const WinMerge a)
{
    constexpr int NC = D - 1;                    // Cb, Cr (and A)
    __shared__ float s_patch[NC][kPatchH][kPatchW];
    __shared__ float s_mid[NC][kTileH][kPatchW];
    __shared__ int s_span[4];
    const int tid = (int)threadIdx.x;
    const unsigned tx = blockIdx.x * kTileW, ty = blockIdx.y * kTileH;       // the tile inside the band
    const int ncol = (int)min((unsigned)kTileW, a.rw - tx), nrow = (int)min((unsigned)kTileH, a.rows - ty);
    const unsigned gx = a.x0 + tx, gy = a.gy0 + ty;                          // the tile inside the dw x dh output

    // 1. - 3. (srcnn_window_tile.h); a staged sample is the split Cb, Cr (and A) of a source pixel
    const TilePatch p = tile_patch(a.t, s_span, tid, gx, gy, ncol, nrow, a.w, a.h);
    tile_stage<NC>(s_patch, p, tid, [&](size_t sr, size_t sc, float* v) {
        float ch[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const unsigned char* q = PLANAR ? a.sp[k] + sr * a.spitch[k] + sc * BPS : a.sp[0] + sr * a.spitch[0] + (sc * D + k) * BPS;
            ch[k] = (float)(load_scalar<BPS>(q) & a.mask) * a.down;
        }
        const float r_ = a.bgr ? ch[2] : ch[0], g = ch[1], b = a.bgr ? ch[0] : ch[2];
        v[0] = split_cb(r_, g, b);
        v[1] = split_cr(r_, g, b);
        if constexpr (D == 4) v[2] = ch[3];
    });
    __syncthreads();
    tile_vertical<NC>(a.t, s_patch, s_mid, p, tid, gy, nrow);
    __syncthreads();

    // 4. horizontal pass, merge, store: 4 consecutive pixels of one row per thread
    const int ry = tid / (kTileW / (int)kChunk), c = (tid % (kTileW / (int)kChunk)) * (int)kChunk;
    if (ry >= nrow || c >= ncol) return;
    const unsigned n = (unsigned)min((int)kChunk, ncol - c);
    const size_t br = (size_t)ty + ry;                       // row of the band
    const size_t dr = (size_t)a.row0 + br;                   // row of the rect = destination row
    const size_t dc = (size_t)tx + c;                        // column of the rect = destination column
    unsigned code[kChunk][D], cv[kChunk];                    // [pixel][channel in memory order]
#pragma unroll
    for (int px = 0; px < (int)kChunk; ++px) {
        float rs[3] = {128.f, 128.f, 0.f};
        float fy = 0.f;
        if ((unsigned)px < n) {
            tile_horizontal<NC>(a.t, s_mid, p, ry, gx + c + px, rs);
            fy = a.y[br * a.rw + dc + px];
        }
        const float cb = rs[0] - 128.f, cr = rs[1] - 128.f;
        const unsigned R = to_code(merge_r(fy, cr), a.up);
        const unsigned G = to_code(merge_g(fy, cb, cr), a.up);
        const unsigned B = to_code(merge_b(fy, cb), a.up);
        code[px][0] = a.bgr ? B : R;
        code[px][1] = G;
        code[px][2] = a.bgr ? R : B;
        if constexpr (D == 4) code[px][3] = to_code(rs[2], a.up);
        cv[px] = (unsigned)(fy * a.up);
    }
    if (n == kChunk && a.int_vec) {
        if constexpr (PLANAR) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                unsigned wd[BPS] = {};
#pragma unroll
                for (int px = 0; px < (int)kChunk; ++px) put_sample<BPS>(wd, px, code[px][k]);
                unsigned* q = reinterpret_cast<unsigned*>(a.dp[k] + dr * a.dpitch[k] + dc * BPS);
#pragma unroll
                for (int t = 0; t < BPS; ++t) q[t] = wd[t];
            }
        } else {
            unsigned wd[D * BPS] = {};
#pragma unroll
            for (int px = 0; px < (int)kChunk; ++px)
#pragma unroll
                for (int k = 0; k < D; ++k) put_sample<BPS>(wd, px * D + k, code[px][k]);
            unsigned* q = reinterpret_cast<unsigned*>(a.dp[0] + dr * a.dpitch[0] + dc * D * BPS);
#pragma unroll
            for (int t = 0; t < D * BPS; ++t) q[t] = wd[t];
        }
    } else {
#pragma unroll
        for (int px = 0; px < (int)kChunk; ++px)
#pragma unroll
            for (int k = 0; k < D; ++k)
                if ((unsigned)px < n) {
                    unsigned char* q = PLANAR ? a.dp[k] + dr * a.dpitch[k] + (dc + px) * BPS
                                              : a.dp[0] + dr * a.dpitch[0] + ((dc + px) * D + k) * BPS;
                    store_scalar<BPS>(q, code[px][k]);
                }
    }
    if (a.conv) {
        unsigned char* q = a.conv + dr * a.conv_pitch + dc * BPS;
        if (n == kChunk && a.conv_vec) {
            unsigned wd[BPS] = {};
#pragma unroll
            for (int px = 0; px < (int)kChunk; ++px) put_sample<BPS>(wd, px, cv[px]);
#pragma unroll
            for (int t = 0; t < BPS; ++t) reinterpret_cast<unsigned*>(q)[t] = wd[t];
        } else {
#pragma unroll
            for (int px = 0; px < (int)kChunk; ++px)
                if ((unsigned)px < n) store_scalar<BPS>(q + (size_t)px * BPS, cv[px]);
        }
    }
}

}  // namespace

void launch_rgb_window_y(const RgbRule& f, const unsigned char* const src[4], const size_t pitch[4], unsigned sx0, unsigned sy0,
                         unsigned sw, unsigned sh, float* y, hipStream_t s)
{
    if (sw == 0 || sh == 0) return;
    WinY a{};
    const int np = f.planar ? 3 : 1;                     // (the alpha plane is not read)
    a.int_vec = 1;
    for (int k = 0; k < np; ++k) {
        a.p[k] = src[k] + (size_t)sy0 * pitch[k] + (size_t)sx0 * f.bps * (f.planar ? 1 : f.ch);
        a.pitch[k] = pitch[k];
        a.int_vec = a.int_vec && aligned_to(a.p[k], 4) && pitch[k] % 4 == 0;
    }
    a.y = y;
    a.flt_vec = sw % 4 == 0 && aligned_to(y, 16);
    a.w = sw; a.rows = sh;
    a.mask = f.mask; a.down = f.down; a.bgr = f.bgr ? 1 : 0;
    const dim3 grid = grid_for((size_t)((sw + kChunk - 1) / kChunk) * sh, 8192);
    RGB_DISPATCH(k_rgb_window_y, f, grid, s, a);
}

void launch_rgb_window_merge(const RgbRule& f, const unsigned char* const src[4], const size_t spitch[4], unsigned w, unsigned h,
                             const float* yband, unsigned x0, unsigned gy0, unsigned rw, unsigned rows,
                             const DevAxisTable& th, const DevAxisTable& tv, unsigned char* const dst[4], const size_t dpitch[4],
                             unsigned row0, unsigned char* conv, size_t conv_pitch, hipStream_t s)
{
    if (rw == 0 || rows == 0) return;
    WinMerge a{};
    const int np = f.planar ? f.ch : 1;
    a.int_vec = 1;
    for (int k = 0; k < np; ++k) {
        a.sp[k] = src[k]; a.spitch[k] = spitch[k];
        a.dp[k] = dst[k]; a.dpitch[k] = dpitch[k];
        a.int_vec = a.int_vec && aligned_to(dst[k], 4) && dpitch[k] % 4 == 0;
    }
    a.conv = conv; a.conv_pitch = conv_pitch;
    a.conv_vec = conv && aligned_to(conv, 4) && conv_pitch % 4 == 0;
    a.y = yband;
    a.x0 = x0; a.gy0 = gy0; a.row0 = row0; a.rw = rw; a.rows = rows; a.w = w; a.h = h;
    a.t = tile_tables(th, tv);
    a.mask = f.mask; a.down = f.down; a.up = f.up; a.bgr = f.bgr ? 1 : 0;
    const dim3 grid((rw + kTileW - 1) / kTileW, (rows + kTileH - 1) / kTileH);
    RGB_DISPATCH(k_rgb_window_merge, f, grid, s, a);
}

}  // namespace srcnn
