// srcnn_rgb_window.hip -- the colour shell of the RGB(A) rect call (include/srcnn_amd_rgb_rect.h) over a WINDOW of the image:
// what srcnn_rgb.hip does for whole rows of whole planes, at the cost of the rect.
//
//   k_rgb_window_y       a rectangle of the integer source plane(s) -> a tight float32 Y window (the source of the window Y
//                        path, y_path_rect): the read rules and the Y line of k_rgb_unpack, nothing else stored -- the Y path
//                        needs the 6-sample halo, chroma does not
//   k_rgb_window_merge   one launch per band: Cb', Cr' (and A') of a 64 x 16 tile of the rect resampled straight from the
//                        integer source, merged with the finished Y' rows and written in the caller's format (and the
//                        truncated Y' plane): split of k_rgb_unpack -> the two passes of k_win_cols / k_win_rows -> merge and
//                        to_code of k_rgb_pack, with that kernel's vector / scalar stores
//
// k_rgb_window_merge serves up-scales in both axes with contribution tables of at most 8 taps (the host checks that every
// tile's source patch fits kPatchW x kPatchH: rgb_window_merge_fits); everything else takes the plane route of rgb_rect
// (srcnn_frames.cpp), which needs no kernel of its own.  A workgroup
//   1. reads the first / last tap of its columns and rows off the tables (LDS min / max): the source patch of the tile,
//   2. stages split Cb, Cr (and A) of the patch in LDS as floats,
//   3. runs the vertical pass into an fp32 intermediate of 16 rows x patch columns (the pass order and the rounded
//      intermediate of resample_window for an up-scale),
//   4. runs the horizontal pass for 4 consecutive pixels per thread, merges them with Y' and stores them.
// Both passes are acc = 0.0; acc = acc + wt[t] * (double)px in tap order; one (float)acc -- the operations of
// k_resample_cols / k_resample_rows, so the tile holds the bits the plane resamplers put at the same place.  The tap count
// of the vertical pass is uniform over a row of the tile; at 2x two neighbouring columns of the horizontal pass read the same
// LDS words (a broadcast), and the 4 rows a wave covers lie kPatchW = 72 words = 8 banks apart.
//
// Every index is bounded: the patch is clamped to the w x h source, LDS indices lie inside the extents the host checked, and a
// thread stores only pixels of its tile that lie inside the rect.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "srcnn_pixel_io.h"
#include "srcnn_rgb.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr unsigned kChunk = 4;                   // pixels per thread
constexpr int kTileW = 64, kTileH = 16;          // the tile of the layer kernels
constexpr int kPatchW = kTileW + 8, kPatchH = kTileH + 8;

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
    const int* hf; const int* ht; const double* hw; int hstride;     // horizontal table (dw <- w)
    const int* vf; const int* vt; const double* vw; int vstride;     // vertical table (dh <- h)
    unsigned mask;
    float down, up;
    int bgr, int_vec, conv_vec;
};

__device__ __forceinline__ unsigned to_code(float v, float up)
{   // as k_rgb_pack: MIN(255.f, v) then MAX(0.f, .) in the reference's macro forms, the exact scaling, the truncating cast
    v = (255.f < v) ? 255.f : v;
    v = (0.f > v) ? 0.f : v;
    return (unsigned)(v * up);
}

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
            yv[px] = (0.299f * r_) + (0.587f * g) + (0.114f * b);                 // src/libsrcnn.cpp:251-256
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

    // 1. the source patch of the tile, off the tables
    if (tid == 0) { s_span[0] = 0x7fffffff; s_span[1] = 0; s_span[2] = 0x7fffffff; s_span[3] = 0; }
    __syncthreads();
    if (tid < ncol) {
        const int f = a.hf[gx + tid];
        atomicMin(&s_span[0], f);
        atomicMax(&s_span[1], f + a.ht[gx + tid]);
    } else if (tid >= kTileW && tid - kTileW < nrow) {
        const int f = a.vf[gy + (tid - kTileW)];
        atomicMin(&s_span[2], f);
        atomicMax(&s_span[3], f + a.vt[gy + (tid - kTileW)]);
    }
    __syncthreads();
    const int c_lo = max(s_span[0], 0), r_lo = max(s_span[2], 0);
    const int pw = min(min(s_span[1], (int)a.w) - c_lo, kPatchW), ph = min(min(s_span[3], (int)a.h) - r_lo, kPatchH);

    // 2. split Cb, Cr (and A) of the patch
    for (int i = tid; i < pw * ph; i += 256) {
        const int pr = i / pw, pc = i - pr * pw;
        const size_t sr = (size_t)(r_lo + pr), sc = (size_t)(c_lo + pc);
        float ch[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const unsigned char* q = PLANAR ? a.sp[k] + sr * a.spitch[k] + sc * BPS : a.sp[0] + sr * a.spitch[0] + (sc * D + k) * BPS;
            ch[k] = (float)(load_scalar<BPS>(q) & a.mask) * a.down;
        }
        const float r_ = a.bgr ? ch[2] : ch[0], g = ch[1], b = a.bgr ? ch[0] : ch[2];
        s_patch[0][pr][pc] = 128.f - (0.1687f * r_) - (0.3313f * g) + (0.5f * b);       // src/libsrcnn.cpp:251-256
        s_patch[1][pr][pc] = 128.f + (0.5f * r_) - (0.4187f * g) - (0.0813f * b);
        if constexpr (D == 4) s_patch[2][pr][pc] = ch[3];
    }
    __syncthreads();

    // 3. vertical pass: rows of the tile x columns of the patch
    for (int i = tid; i < nrow * pw; i += 256) {
        const int ry = i / pw, pc = i - ry * pw;
        const unsigned y = gy + ry;
        const int s0 = a.vf[y] - r_lo, n = a.vt[y];
        const double* wr = a.vw + (size_t)y * a.vstride;
        if (s0 < 0 || s0 + n > kPatchH) continue;            // (never: rgb_window_merge_fits)
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            double acc = 0.0;
            for (int t = 0; t < n; ++t) {
                const double px = (double)s_patch[k][s0 + t][pc];
                acc = acc + wr[t] * px;
            }
            s_mid[k][ry][pc] = (float)acc;
        }
    }
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
            const unsigned x = gx + c + px;
            const int s0 = a.hf[x] - c_lo, nt = a.ht[x];
            const double* wr = a.hw + (size_t)x * a.hstride;
            if (s0 >= 0 && s0 + nt <= kPatchW) {             // (always: rgb_window_merge_fits)
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    double acc = 0.0;
                    for (int t = 0; t < nt; ++t) acc = acc + wr[t] * (double)s_mid[k][ry][s0 + t];
                    rs[k] = (float)acc;
                }
            }
            fy = a.y[br * a.rw + dc + px];
        }
        const float cb = rs[0] - 128.f, cr = rs[1] - 128.f;                      // src/libsrcnn.cpp:287-307
        const unsigned R = to_code(fy + 45.f * cr / 32.f, a.up);
        const unsigned G = to_code(fy - (11.f * cb + 23.f * cr) / 32.f, a.up);
        const unsigned B = to_code(fy + 113.f * cb / 64.f, a.up);
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

#define RGB_WINDOW_DISPATCH(KERNEL, f, grid, s, a)                                                                           \
    do {                                                                                                                     \
        const int sel = ((f).bps == 2 ? 4 : 0) | ((f).planar ? 2 : 0) | ((f).ch == 4 ? 1 : 0);                               \
        switch (sel) {                                                                                                       \
        case 0: hipLaunchKernelGGL((KERNEL<1, false, 3>), grid, dim3(256), 0, s, a); break;                                  \
        case 1: hipLaunchKernelGGL((KERNEL<1, false, 4>), grid, dim3(256), 0, s, a); break;                                  \
        case 2: hipLaunchKernelGGL((KERNEL<1, true, 3>), grid, dim3(256), 0, s, a); break;                                   \
        case 3: hipLaunchKernelGGL((KERNEL<1, true, 4>), grid, dim3(256), 0, s, a); break;                                   \
        case 4: hipLaunchKernelGGL((KERNEL<2, false, 3>), grid, dim3(256), 0, s, a); break;                                  \
        case 5: hipLaunchKernelGGL((KERNEL<2, false, 4>), grid, dim3(256), 0, s, a); break;                                  \
        case 6: hipLaunchKernelGGL((KERNEL<2, true, 3>), grid, dim3(256), 0, s, a); break;                                   \
        default: hipLaunchKernelGGL((KERNEL<2, true, 4>), grid, dim3(256), 0, s, a); break;                                  \
        }                                                                                                                    \
    } while (0)

// the extent of source indices that `count` destination indices from `first` read, tile by tile of `tile` of them, fits `cap`
bool axis_tiles_fit(const DevAxisTable& t, unsigned first, unsigned count, unsigned tile, int cap)
{
    if (!t.h_first || !t.h_taps || t.max_taps > 8) return false;
    for (unsigned a = 0; a < count; a += tile) {
        int lo = 0x7fffffff, hi = 0;
        for (unsigned u = first + a; u < first + std::min(count, a + tile); ++u) {
            lo = std::min(lo, t.h_first[u]);
            hi = std::max(hi, t.h_first[u] + t.h_taps[u]);
        }
        if (lo < 0 || hi - lo > cap) return false;
    }
    return true;
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
    RGB_WINDOW_DISPATCH(k_rgb_window_y, f, grid, s, a);
}

bool rgb_window_merge_fits(const DevAxisTable& th, const DevAxisTable& tv, unsigned x0, unsigned rw, unsigned gy0, unsigned rows)
{
    return axis_tiles_fit(th, x0, rw, kTileW, kPatchW) && axis_tiles_fit(tv, gy0, rows, kTileH, kPatchH);
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
    a.hf = th.first; a.ht = th.taps; a.hw = th.weight; a.hstride = th.stride;
    a.vf = tv.first; a.vt = tv.taps; a.vw = tv.weight; a.vstride = tv.stride;
    a.mask = f.mask; a.down = f.down; a.up = f.up; a.bgr = f.bgr ? 1 : 0;
    const dim3 grid((rw + kTileW - 1) / kTileW, (rows + kTileH - 1) / kTileH);
    RGB_WINDOW_DISPATCH(k_rgb_window_merge, f, grid, s, a);
}

}  // namespace srcnn
