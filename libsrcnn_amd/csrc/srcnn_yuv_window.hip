// srcnn_yuv_window.hip -- the chroma of the YUV rect call (include/srcnn_amd_yuv_rect.h) over a WINDOW of the frame: what
// k_plane_unpack -> the plane resamplers -> k_plane_pack (srcnn_yuv_planes.hip) do for whole chroma planes, at the cost of the
// rect and without a float chroma plane.
//
//   k_yuv_window_chroma   one launch per rect: U' and V' of a 64 x 16 tile of the chroma rect resampled straight from the
//                         integer source and written in the caller's format: the read rule of k_plane_unpack (16-bit words:
//                         word_value, on the native scale) -> the tile resampler (srcnn_window_tile.h, which describes its four
//                         steps and says which shapes it serves; here on the CHROMA grid: dcw > cw and dch > ch) -> the
//                         saturation and the write rule of k_plane_pack.  Planar: two source and two destination planes;
//                         semi-planar: one plane of (U, V) pairs, de-interleaved on the way in and interleaved on the way out.
//
// The pixel rules are srcnn_colour_rules.h, shared with srcnn_yuv_planes.hip.  A thread stores only samples of its tile that lie
// inside the chroma rect.  Its 4 samples (4 pairs) go out as one 4- / 8- / 16-byte store where the plane's base and pitch are
// multiples of that size, else sample by sample.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_window_tile.h"
#include "srcnn_yuv.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr unsigned kChunk = kTileChunk;          // samples per thread and plane

struct WinChroma {
    const unsigned char* sp[2];                  // the WHOLE source chroma planes (semi-planar: sp[0] only)
    size_t spitch[2];
    unsigned char* dp[2];                        // destination planes: chroma sample (cx0, cy0) first
    size_t dpitch[2];
    unsigned cx0, cy0;                           // the chroma rect inside the dcw x dch chroma output
    unsigned cols, rows;
    unsigned w, h;                               // source chroma size (cw x ch)
    TileTables t;                                // horizontal table (dcw <- cw), vertical table (dch <- ch)
    unsigned rshift, mask, lshift;               // 16-bit words: read (word >> rshift) & mask, write value << lshift
    float maxv;
    int dst_vec;
};

template <int BPS>
__device__ __forceinline__ float chroma_in(const unsigned char* q, unsigned rshift, unsigned mask)
{
    if constexpr (BPS == 1) return (float)load_scalar<1>(q);
    else return (float)word_value(load_scalar<2>(q), rshift, mask);
}

// ND dwords at p as ONE store (p is aligned to 4 * ND bytes)
template <unsigned ND>
__device__ __forceinline__ void store_chunk(unsigned char* p, const unsigned* q)
{
    typedef unsigned uvec2 __attribute__((ext_vector_type(2)));
    typedef unsigned uvec4 __attribute__((ext_vector_type(4)));
    if constexpr (ND == 1) *reinterpret_cast<unsigned*>(p) = q[0];
    else if constexpr (ND == 2) *reinterpret_cast<uvec2*>(p) = uvec2{q[0], q[1]};
    else *reinterpret_cast<uvec4*>(p) = uvec4{q[0], q[1], q[2], q[3]};
}

template <int BPS, bool SEMI>
__global__ __launch_bounds__(256) void k_yuv_window_chroma(const WinChroma a)
{
    constexpr unsigned SPP = SEMI ? 2 : 1;                   // samples per column of a plane
    constexpr unsigned ND = kChunk * BPS * SPP / 4;          // dwords of a thread's chunk in one plane
    __shared__ float s_patch[2][kPatchH][kPatchW];
    __shared__ float s_mid[2][kTileH][kPatchW];
    __shared__ int s_span[4];
    const int tid = (int)threadIdx.x;
    const unsigned tx = blockIdx.x * kTileW, ty = blockIdx.y * kTileH;       // the tile inside the chroma rect
    const int ncol = (int)min((unsigned)kTileW, a.cols - tx), nrow = (int)min((unsigned)kTileH, a.rows - ty);
    const unsigned gx = a.cx0 + tx, gy = a.cy0 + ty;                         // the tile inside the dcw x dch chroma output

    // 1. - 3. (srcnn_window_tile.h); a staged sample is U and V of a source column
    const TilePatch p = tile_patch(a.t, s_span, tid, gx, gy, ncol, nrow, a.w, a.h);
    tile_stage<2>(s_patch, p, tid, [&](size_t sr, size_t sc, float* v) {
        const unsigned char* qu = a.sp[0] + sr * a.spitch[0] + sc * SPP * BPS;
        const unsigned char* qv = SEMI ? qu + BPS : a.sp[1] + sr * a.spitch[1] + sc * BPS;
        v[0] = chroma_in<BPS>(qu, a.rshift, a.mask);
        v[1] = chroma_in<BPS>(qv, a.rshift, a.mask);
    });
    __syncthreads();
    tile_vertical<2>(a.t, s_patch, s_mid, p, tid, gy, nrow);
    __syncthreads();

    // 4. horizontal pass, saturate, store: 4 consecutive samples of one row per thread
    const int ry = tid / (kTileW / (int)kChunk), c = (tid % (kTileW / (int)kChunk)) * (int)kChunk;
    if (ry >= nrow || c >= ncol) return;
    const unsigned n = (unsigned)min((int)kChunk, ncol - c);
    const size_t dr = (size_t)ty + ry;                       // row of the chroma rect = destination row
    const size_t dc = (size_t)tx + c;                        // column of the chroma rect = destination column
    unsigned code[2][kChunk];
#pragma unroll
    for (int px = 0; px < (int)kChunk; ++px) {
        float rs[2] = {0.f, 0.f};
        if ((unsigned)px < n) tile_horizontal<2>(a.t, s_mid, p, ry, gx + c + px, rs);
        code[0][px] = to_saturated_sample<BPS>(rs[0], a.maxv, a.lshift);
        code[1][px] = to_saturated_sample<BPS>(rs[1], a.maxv, a.lshift);
    }
    if (n == kChunk && a.dst_vec) {
        if constexpr (SEMI) {
            unsigned wd[ND] = {};
#pragma unroll
            for (int px = 0; px < (int)kChunk; ++px) { put_sample<BPS>(wd, 2 * px, code[0][px]); put_sample<BPS>(wd, 2 * px + 1, code[1][px]); }
            store_chunk<ND>(a.dp[0] + dr * a.dpitch[0] + dc * SPP * BPS, wd);
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                unsigned wd[ND] = {};
#pragma unroll
                for (int px = 0; px < (int)kChunk; ++px) put_sample<BPS>(wd, px, code[k][px]);
                store_chunk<ND>(a.dp[k] + dr * a.dpitch[k] + dc * BPS, wd);
            }
        }
    } else {
#pragma unroll
        for (int px = 0; px < (int)kChunk; ++px)
            if ((unsigned)px < n) {
                unsigned char* qu = a.dp[0] + dr * a.dpitch[0] + (dc + px) * SPP * BPS;
                unsigned char* qv = SEMI ? qu + BPS : a.dp[1] + dr * a.dpitch[1] + (dc + px) * BPS;
                store_scalar<BPS>(qu, code[0][px]);
                store_scalar<BPS>(qv, code[1][px]);
            }
    }
}

}  // namespace

void launch_yuv_window_chroma(const unsigned char* const src[2], const size_t spitch[2], unsigned cw, unsigned ch, bool semi,
                              const Yuv16Rule* f, unsigned cx0, unsigned cy0, unsigned cols, unsigned rows, const DevAxisTable& th,
                              const DevAxisTable& tv, unsigned char* const dst[2], const size_t dpitch[2], hipStream_t s)
{
    if (cols == 0 || rows == 0) return;
    WinChroma a{};
    const size_t chunk = (size_t)kChunk * (f ? 2 : 1) * (semi ? 2 : 1);      // bytes of a thread's store
    a.dst_vec = 1;
    for (int k = 0; k < (semi ? 1 : 2); ++k) {
        a.sp[k] = src[k]; a.spitch[k] = spitch[k];
        a.dp[k] = dst[k]; a.dpitch[k] = dpitch[k];
        a.dst_vec = a.dst_vec && aligned_to(dst[k], chunk) && dpitch[k] % chunk == 0;
    }
    a.cx0 = cx0; a.cy0 = cy0; a.cols = cols; a.rows = rows; a.w = cw; a.h = ch;
    a.t = tile_tables(th, tv);
    a.rshift = f ? f->rshift : 0; a.mask = f ? f->mask : 0xffu; a.lshift = f ? f->lshift : 0;
    a.maxv = f ? (float)f->mask : 255.f;
    const dim3 grid((cols + kTileW - 1) / kTileW, (rows + kTileH - 1) / kTileH);
    switch ((f ? 2 : 0) | (semi ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((k_yuv_window_chroma<1, false>), grid, dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL((k_yuv_window_chroma<1, true>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_yuv_window_chroma<2, false>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((k_yuv_window_chroma<2, true>), grid, dim3(256), 0, s, a); break;
    }
}

}  // namespace srcnn
