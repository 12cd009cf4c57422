// srcnn_rgb.hip -- the conversions around the SRCNN path for RGB(A) images that live in device memory
// (include/srcnn_amd_rgb.h): interleaved or planar samples, 8-bit or 16-bit words, either channel order, pitched rows.
//
//   k_rgb_unpack   integer plane(s) -> tight float32 planes Y, Cb, Cr (and A)
//                  value = word & maxv;  R, G, B, A = (float)value * 2^-s (exact);  then the split of k_rgb_split
//                  (src/libsrcnn.cpp:233-272): every product and every sum rounded on its own, no contraction
//   k_rgb_pack     tight float32 rows Y', Cb', Cr' (and A') -> destination rows of the integer plane(s), and optionally the
//                  truncated Y' plane; the merge of k_ycc_merge (src/libsrcnn.cpp:274-308), then
//                  sample = (unsigned)(MAX(0, MIN(255, v)) * 2^s) in the reference's macro forms
// The split, the merge and the sample code are srcnn_colour_rules.h, shared with the window kernels of srcnn_rgb_window.hip.
//
// Both kernels are memory-bound and move 4 pixels per thread: the float side as one 16-byte access per plane, the integer
// side as the 1 .. 8 consecutive dwords that hold the 4 pixels (12 / 16 / 24 / 32 bytes interleaved, 4 / 8 bytes per plane
// planar; consecutive dwords are merged into wider accesses by the compiler), where bases and pitches are aligned for it
// (decided once per launch); a row's last partial chunk and misaligned planes take the scalar forms, so that no byte outside a
// row's samples is ever touched.  Grid-stride over rows x chunks.  mask and the two scalings are kernel arguments: every depth
// runs the same instances.  The host side is srcnn_frames.cpp (rgb_frame).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_rgb.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr unsigned kChunkRgb = 4;        // pixels per thread

struct RgbIo {
    unsigned char* p[4];                 // integer planes (interleaved: p[0] only)
    size_t pitch[4];
    float* f[4];                         // float planes Y, Cb, Cr, A: tight, w floats per row
    unsigned char* conv;                 // pack only: truncated Y', or NULL
    size_t conv_pitch;
    unsigned w, rows, row0;              // row0: pack only, the destination row of float row 0
    unsigned mask;
    float down, up;
    int bgr;
    int int_vec, flt_vec, conv_vec;      // dword accesses of the integer planes / float4 accesses / dword stores of conv are aligned
};

template <int BPS, bool PLANAR, int D>
__global__ __launch_bounds__(256) void k_rgb_unpack(const RgbIo a)
{
    const unsigned cpr = (a.w + kChunkRgb - 1) / kChunkRgb;
    const unsigned total = cpr * a.rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * kChunkRgb;
        const unsigned n = min(kChunkRgb, a.w - c);
        unsigned v[kChunkRgb][D];        // [pixel][channel in memory order]
        if (n == kChunkRgb && a.int_vec) {
            if constexpr (PLANAR) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const unsigned* q = reinterpret_cast<const unsigned*>(a.p[k] + (size_t)r * a.pitch[k] + (size_t)c * BPS);
                    unsigned wd[BPS];
#pragma unroll
                    for (int t = 0; t < BPS; ++t) wd[t] = q[t];
#pragma unroll
                    for (int px = 0; px < (int)kChunkRgb; ++px) v[px][k] = sample_of<BPS>(wd, px);
                }
            } else {
                const unsigned* q = reinterpret_cast<const unsigned*>(a.p[0] + (size_t)r * a.pitch[0] + (size_t)c * D * BPS);
                unsigned wd[D * BPS];
#pragma unroll
                for (int t = 0; t < D * BPS; ++t) wd[t] = q[t];
#pragma unroll
                for (int px = 0; px < (int)kChunkRgb; ++px)
#pragma unroll
                    for (int k = 0; k < D; ++k) v[px][k] = sample_of<BPS>(wd, px * D + k);
            }
        } else {
#pragma unroll
            for (int px = 0; px < (int)kChunkRgb; ++px)
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    v[px][k] = 0;
                    if ((unsigned)px < n) {
                        const unsigned char* q = PLANAR ? a.p[k] + (size_t)r * a.pitch[k] + (size_t)(c + px) * BPS
                                                        : a.p[0] + (size_t)r * a.pitch[0] + ((size_t)(c + px) * D + k) * BPS;
                        v[px][k] = load_scalar<BPS>(q);
                    }
                }
        }
        float yv[kChunkRgb], cbv[kChunkRgb], crv[kChunkRgb], av[kChunkRgb];
#pragma unroll
        for (int px = 0; px < (int)kChunkRgb; ++px) {
            float ch[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < D; ++k) ch[k] = (float)(v[px][k] & a.mask) * a.down;
            const float r_ = a.bgr ? ch[2] : ch[0], g = ch[1], b = a.bgr ? ch[0] : ch[2];
            yv[px] = split_y(r_, g, b);
            cbv[px] = split_cb(r_, g, b);
            crv[px] = split_cr(r_, g, b);
            av[px] = ch[3];
        }
        const size_t o = (size_t)r * a.w + c;
        if (n == kChunkRgb && a.flt_vec) {
            store_floats_vec<kChunkRgb>(a.f[0] + o, yv);
            store_floats_vec<kChunkRgb>(a.f[1] + o, cbv);
            store_floats_vec<kChunkRgb>(a.f[2] + o, crv);
            if constexpr (D == 4) store_floats_vec<kChunkRgb>(a.f[3] + o, av);
        } else {
#pragma unroll
            for (int px = 0; px < (int)kChunkRgb; ++px) {
                if ((unsigned)px < n) {
                    a.f[0][o + px] = yv[px];
                    a.f[1][o + px] = cbv[px];
                    a.f[2][o + px] = crv[px];
                    if constexpr (D == 4) a.f[3][o + px] = av[px];
                }
            }
        }
    }
}

template <int BPS, bool PLANAR, int D>
__global__ __launch_bounds__(256) void k_rgb_pack(const RgbIo a)
{
    const unsigned cpr = (a.w + kChunkRgb - 1) / kChunkRgb;
    const unsigned total = cpr * a.rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = (i - r * cpr) * kChunkRgb;
        const unsigned n = min(kChunkRgb, a.w - c);
        const size_t o = (size_t)r * a.w + c;
        const size_t dr = (size_t)a.row0 + r;                    // destination row
        float yv[kChunkRgb], cbv[kChunkRgb], crv[kChunkRgb], av[kChunkRgb] = {0.f, 0.f, 0.f, 0.f};
        load_floats<kChunkRgb>(a.f[0] + o, yv, n, a.flt_vec);
        load_floats<kChunkRgb>(a.f[1] + o, cbv, n, a.flt_vec);
        load_floats<kChunkRgb>(a.f[2] + o, crv, n, a.flt_vec);
        if constexpr (D == 4) load_floats<kChunkRgb>(a.f[3] + o, av, n, a.flt_vec);
        unsigned code[kChunkRgb][D], cv[kChunkRgb];              // [pixel][channel in memory order]
#pragma unroll
        for (int px = 0; px < (int)kChunkRgb; ++px) {
            const float fy = yv[px], cb = cbv[px] - 128.f, cr = crv[px] - 128.f;
            const unsigned R = to_code(merge_r(fy, cr), a.up);
            const unsigned G = to_code(merge_g(fy, cb, cr), a.up);
            const unsigned B = to_code(merge_b(fy, cb), a.up);
            code[px][0] = a.bgr ? B : R;
            code[px][1] = G;
            code[px][2] = a.bgr ? R : B;
            if constexpr (D == 4) code[px][3] = to_code(av[px], a.up);
            cv[px] = (unsigned)(fy * a.up);
        }
        if (n == kChunkRgb && a.int_vec) {
            if constexpr (PLANAR) {
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    unsigned wd[BPS] = {};
#pragma unroll
                    for (int px = 0; px < (int)kChunkRgb; ++px) put_sample<BPS>(wd, px, code[px][k]);
                    unsigned* q = reinterpret_cast<unsigned*>(a.p[k] + dr * a.pitch[k] + (size_t)c * BPS);
#pragma unroll
                    for (int t = 0; t < BPS; ++t) q[t] = wd[t];
                }
            } else {
                unsigned wd[D * BPS] = {};
#pragma unroll
                for (int px = 0; px < (int)kChunkRgb; ++px)
#pragma unroll
                    for (int k = 0; k < D; ++k) put_sample<BPS>(wd, px * D + k, code[px][k]);
                unsigned* q = reinterpret_cast<unsigned*>(a.p[0] + dr * a.pitch[0] + (size_t)c * D * BPS);
#pragma unroll
                for (int t = 0; t < D * BPS; ++t) q[t] = wd[t];
            }
        } else {
#pragma unroll
            for (int px = 0; px < (int)kChunkRgb; ++px)
#pragma unroll
                for (int k = 0; k < D; ++k)
                    if ((unsigned)px < n) {
                        unsigned char* q = PLANAR ? a.p[k] + dr * a.pitch[k] + (size_t)(c + px) * BPS
                                                  : a.p[0] + dr * a.pitch[0] + ((size_t)(c + px) * D + k) * BPS;
                        store_scalar<BPS>(q, code[px][k]);
                    }
        }
        if (a.conv) {
            unsigned char* q = a.conv + dr * a.conv_pitch + (size_t)c * BPS;
            if (n == kChunkRgb && a.conv_vec) {
                unsigned wd[BPS] = {};
#pragma unroll
                for (int px = 0; px < (int)kChunkRgb; ++px) put_sample<BPS>(wd, px, cv[px]);
#pragma unroll
                for (int t = 0; t < BPS; ++t) reinterpret_cast<unsigned*>(q)[t] = wd[t];
            } else {
#pragma unroll
                for (int px = 0; px < (int)kChunkRgb; ++px)
                    if ((unsigned)px < n) store_scalar<BPS>(q + (size_t)px * BPS, cv[px]);
            }
        }
    }
}

dim3 rgb_grid(unsigned w, unsigned rows) { return grid_for((size_t)((w + kChunkRgb - 1) / kChunkRgb) * rows, 8192); }

RgbIo io_of(const RgbRule& f, unsigned char* const p[4], const size_t pitch[4], float* const fl[4], unsigned w, unsigned rows)
{
    RgbIo a{};
    const int np = f.planar ? f.ch : 1;
    a.int_vec = 1;
    for (int k = 0; k < np; ++k) {
        a.p[k] = p[k]; a.pitch[k] = pitch[k];
        a.int_vec = a.int_vec && aligned_to(p[k], 4) && pitch[k] % 4 == 0;
    }
    a.flt_vec = w % 4 == 0;
    for (int k = 0; k < f.ch; ++k) {
        a.f[k] = fl[k];
        a.flt_vec = a.flt_vec && aligned_to(fl[k], 16);
    }
    a.w = w; a.rows = rows;
    a.mask = f.mask; a.down = f.down; a.up = f.up; a.bgr = f.bgr ? 1 : 0;
    return a;
}

}  // namespace

void launch_rgb_unpack(const RgbRule& f, const unsigned char* const src[4], const size_t pitch[4], unsigned w, unsigned rows,
                       float* const out[4], hipStream_t s)
{
    if (w == 0 || rows == 0) return;
    unsigned char* p[4];
    for (int k = 0; k < 4; ++k) p[k] = const_cast<unsigned char*>(src[k]);      // (the unpack kernel only reads them)
    const RgbIo a = io_of(f, p, pitch, out, w, rows);
    const dim3 grid = rgb_grid(w, rows);
    RGB_DISPATCH(k_rgb_unpack, f, grid, s, a);
}

void launch_rgb_pack(const RgbRule& f, const float* const in[4], unsigned w, unsigned rows, unsigned char* const dst[4],
                     const size_t pitch[4], unsigned row0, unsigned char* conv, size_t conv_pitch, hipStream_t s)
{
    if (w == 0 || rows == 0) return;
    float* fl[4];
    for (int k = 0; k < 4; ++k) fl[k] = const_cast<float*>(in[k]);              // (the pack kernel only reads them)
    RgbIo a = io_of(f, dst, pitch, fl, w, rows);
    a.row0 = row0;
    a.conv = conv; a.conv_pitch = conv_pitch;
    a.conv_vec = conv && aligned_to(conv, 4) && conv_pitch % 4 == 0;
    const dim3 grid = rgb_grid(w, rows);
    RGB_DISPATCH(k_rgb_pack, f, grid, s, a);
}

}  // namespace srcnn
