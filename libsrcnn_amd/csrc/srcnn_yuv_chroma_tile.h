// srcnn_yuv_chroma_tile.h -- the body of the tile chroma kernels of planar / semi-planar YUV frames: k_yuv_window_chroma
// (srcnn_yuv_window.hip: one rect per launch) and k_yuv_list_chroma (srcnn_yuv_rect_list.hip: every rect of an atlas per launch)
// instantiate yuv_chroma_tile, as both resample kernels of the rect lists instantiate list_resample_tile (srcnn_rect_list.h).
// What differs between them is how a workgroup finds its rect and its tile.  Internal, HIP only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_window_tile.h"

#pragma clang fp contract(off)

namespace srcnn {

struct ChromaTileSource {
    const unsigned char* sp[2];                  // the WHOLE source chroma planes (semi-planar: sp[0] only)
    size_t spitch[2];
    unsigned w, h;                               // source chroma size (cw x ch)
    TileTables t;                                // horizontal table (dcw <- cw), vertical table (dch <- ch)
    unsigned rshift, mask, lshift;               // 16-bit words: read (word >> rshift) & mask, write value << lshift
    float maxv;
};

struct ChromaTileDst {
    unsigned char* dp[2];                        // destination planes: chroma sample (cx0, cy0) first (semi-planar: dp[0] only)
    size_t dpitch[2];
    unsigned cx0, cy0;                           // the chroma rect inside the dcw x dch chroma output
    unsigned cols, rows;
    int dst_vec;                                 // every plane's base and pitch are multiples of a thread's store
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

// U' and V' of the 64 x 16 tile whose first sample is (tx, ty) of the chroma rect d (tx < d.cols, ty < d.rows: the same for the
// whole workgroup), resampled straight from the integer source and written in the caller's format: the read rule of
// k_plane_unpack -> the tile resampler -> the saturation and the write rule of k_plane_pack.  A thread stores only samples of
// its tile that lie inside the chroma rect; its 4 samples (4 pairs) go out as one 4- / 8- / 16-byte store where d.dst_vec says
// so, else sample by sample.  Four barriers, no return ahead of the last.
template <int BPS, bool SEMI>
__device__ __forceinline__ void yuv_chroma_tile(const ChromaTileSource& a, const ChromaTileDst& d, unsigned tx, unsigned ty)
{
    constexpr unsigned kChunk = kTileChunk;                  // samples per thread and plane
    constexpr unsigned SPP = SEMI ? 2 : 1;                   // samples per column of a plane
    constexpr unsigned ND = kChunk * BPS * SPP / 4;          // dwords of a thread's chunk in one plane
    __shared__ float s_patch[2][kPatchH][kPatchW];
    __shared__ float s_mid[2][kTileH][kPatchW];
    __shared__ int s_span[4];
    const int tid = (int)threadIdx.x;
    const int ncol = (int)min((unsigned)kTileW, d.cols - tx), nrow = (int)min((unsigned)kTileH, d.rows - ty);
    const unsigned gx = d.cx0 + tx, gy = d.cy0 + ty;                         // the tile inside the dcw x dch chroma output

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
    if (n == kChunk && d.dst_vec) {
        if constexpr (SEMI) {
            unsigned wd[ND] = {};
#pragma unroll
            for (int px = 0; px < (int)kChunk; ++px) { put_sample<BPS>(wd, 2 * px, code[0][px]); put_sample<BPS>(wd, 2 * px + 1, code[1][px]); }
            store_chunk<ND>(d.dp[0] + dr * d.dpitch[0] + dc * SPP * BPS, wd);
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                unsigned wd[ND] = {};
#pragma unroll
                for (int px = 0; px < (int)kChunk; ++px) put_sample<BPS>(wd, px, code[k][px]);
                store_chunk<ND>(d.dp[k] + dr * d.dpitch[k] + dc * BPS, wd);
            }
        }
    } else {
#pragma unroll
        for (int px = 0; px < (int)kChunk; ++px)
            if ((unsigned)px < n) {
                unsigned char* qu = d.dp[0] + dr * d.dpitch[0] + (dc + px) * SPP * BPS;
                unsigned char* qv = SEMI ? qu + BPS : d.dp[1] + dr * d.dpitch[1] + (dc + px) * BPS;
                store_scalar<BPS>(qu, code[0][px]);
                store_scalar<BPS>(qv, code[1][px]);
            }
    }
}

}  // namespace srcnn
