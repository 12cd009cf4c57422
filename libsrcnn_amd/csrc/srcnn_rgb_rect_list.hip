// srcnn_rgb_rect_list.hip -- the two kernels that join the colour shell of the RGB(A) rect call to the atlas of the rect LIST
// call (include/srcnn_amd_rgb_rect_list.h).  Between them run the list's own launches, unchanged (srcnn_rect_list.hip and the
// layer kernels).
//
//   k_rgb_list_resample   k_list_resample with an integer fetch: the in-plane part of every cell, resampled by the tile
//                         resampler from Y = split_y of the integer source pixel, read with the rules of k_rgb_window_y
//                         (srcnn_rgb_window.hip).  No float plane of the source image exists.
//   k_rgb_list_merge      k_list_scatter's place: one workgroup takes one 64 x 16 tile of one rect, found by bisection over
//                         sc_tile0, and runs the steps of k_rgb_window_merge on it -- Cb, Cr (and A) of the source patch staged
//                         from the integer planes, the two passes of the tile resampler with the chroma tables, merge and
//                         to_code -- with Y' read from the atlas result.  Stores go to the item's own planes and dst_conv
//                         (ListDstDesc, srcnn_rgb_rect_atlas.hpp), in 4-byte words where that item's bases and pitches allow it.
//
// The pixel rules are srcnn_colour_rules.h.  Every index is bounded: a tile is cut to its rect, the source patch is clamped to
// the w x h image (tile_patch), the cell lies inside the atlas (tests/host/rect_list_sanitize.cpp), and a thread stores only
// pixels of its rect: rw pixels per row, rh rows (tests/host/rgb_rect_list_sanitize.cpp recomputes that range off the descriptor).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_rect_list.h"
#include "srcnn_rgb.h"
#include "srcnn_rgb_rect_atlas.hpp"
#include "srcnn_window_tile.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr unsigned kChunk = kTileChunk;          // pixels per thread of the merge

struct ListSource {
    const unsigned char* sp[4];                  // the WHOLE source planes (interleaved: sp[0] only)
    size_t spitch[4];
    unsigned w, h;
    unsigned mask;
    float down, up;
    int bgr;
};

struct ListResample {
    ListSource src;
    TileTables t;                                // the Y tables: horizontal (dw <- w), vertical (dh <- h)
    const ListCellDesc* d;
    unsigned n;
    float* atlas;
    unsigned atlas_w;
};

struct ListMerge {
    ListSource src;
    TileTables t;                                // the chroma tables
    const ListCellDesc* d;
    const ListDstDesc* dd;                       // entry k: the destination of cell k
    unsigned n;
    const float* atlas;                          // the layer-3 result
    unsigned atlas_w;
};

template <int BPS, bool PLANAR, int D>
__global__ __launch_bounds__(256) void k_rgb_list_resample(const ListResample a)
{
    const ListSource& s = a.src;
    list_resample_tile(s.w, s.h, a.t, a.d, a.n, a.atlas, a.atlas_w, [&](size_t sr, size_t sc, float* v) {
        float ch[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {            // (alpha is not read)
            const unsigned char* q = PLANAR ? s.sp[k] + sr * s.spitch[k] + sc * BPS : s.sp[0] + sr * s.spitch[0] + (sc * D + k) * BPS;
            ch[k] = (float)(load_scalar<BPS>(q) & s.mask) * s.down;
        }
        const float r_ = s.bgr ? ch[2] : ch[0], g = ch[1], b = s.bgr ? ch[0] : ch[2];
        v[0] = split_y(r_, g, b);
    });
}

template <int BPS, bool PLANAR, int D>
__global__ __launch_bounds__(256) void k_rgb_list_merge(const ListMerge a)
{
    constexpr int NC = D - 1;                    // Cb, Cr (and A)
    __shared__ float s_patch[NC][kPatchH][kPatchW];
    __shared__ float s_mid[NC][kTileH][kPatchW];
    __shared__ int s_span[4];
    const ListSource& s = a.src;
    const int tid = (int)threadIdx.x;
    const unsigned cell = find_cell<&ListCellDesc::sc_tile0>(a.d, a.n, blockIdx.x);      // the same for the whole workgroup
    const ListCellDesc c = a.d[cell];
    const unsigned tile = blockIdx.x - c.sc_tile0, tiles_x = (c.rw + kTileW - 1) / kTileW;
    const unsigned tx = (tile % tiles_x) * kTileW, ty = (tile / tiles_x) * kTileH;       // the tile inside the rect
    if (tx >= c.rw || ty >= c.rh) return;                                                // (never: the prefix sums count these tiles)
    const int ncol = (int)min((unsigned)kTileW, c.rw - tx), nrow = (int)min((unsigned)kTileH, c.rh - ty);
    const unsigned gx = c.px + kCellMargin - c.ox + tx, gy = c.py + kCellMargin - c.oy + ty;     // the tile inside the dw x dh output

    // 1. - 3. (srcnn_window_tile.h); a staged sample is the split Cb, Cr (and A) of a source pixel
    const TilePatch p = tile_patch(a.t, s_span, tid, gx, gy, ncol, nrow, s.w, s.h);
    tile_stage<NC>(s_patch, p, tid, [&](size_t sr, size_t sc, float* v) {
        float ch[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const unsigned char* q = PLANAR ? s.sp[k] + sr * s.spitch[k] + sc * BPS : s.sp[0] + sr * s.spitch[0] + (sc * D + k) * BPS;
            ch[k] = (float)(load_scalar<BPS>(q) & s.mask) * s.down;
        }
        const float r_ = s.bgr ? ch[2] : ch[0], g = ch[1], b = s.bgr ? ch[0] : ch[2];
        v[0] = split_cb(r_, g, b);
        v[1] = split_cr(r_, g, b);
        if constexpr (D == 4) v[2] = ch[3];
    });
    __syncthreads();
    tile_vertical<NC>(a.t, s_patch, s_mid, p, tid, gy, nrow);
    __syncthreads();

    // 4. horizontal pass, merge, store: 4 consecutive pixels of one row per thread
    const int ry = tid / (kTileW / (int)kChunk), cc = (tid % (kTileW / (int)kChunk)) * (int)kChunk;
    if (ry >= nrow || cc >= ncol) return;
    const unsigned n = (unsigned)min((int)kChunk, ncol - cc);
    const ListDstDesc o = a.dd[cell];
    const size_t dr = (size_t)ty + ry;                       // row of the rect = destination row
    const size_t dc = (size_t)tx + cc;                       // column of the rect = destination column
    const float* yrow = a.atlas + (size_t)(c.ay + kCellMargin + dr) * a.atlas_w + (c.ax + kCellMargin + dc);
    unsigned code[kChunk][D], cv[kChunk];                    // [pixel][channel in memory order]
#pragma unroll
    for (int px = 0; px < (int)kChunk; ++px) {
        float rs[3] = {128.f, 128.f, 0.f};
        float fy = 0.f;
        if ((unsigned)px < n) {
            tile_horizontal<NC>(a.t, s_mid, p, ry, gx + cc + px, rs);
            fy = yrow[px];
        }
        const float cb = rs[0] - 128.f, cr = rs[1] - 128.f;
        const unsigned R = to_code(merge_r(fy, cr), s.up);
        const unsigned G = to_code(merge_g(fy, cb, cr), s.up);
        const unsigned B = to_code(merge_b(fy, cb), s.up);
        code[px][0] = s.bgr ? B : R;
        code[px][1] = G;
        code[px][2] = s.bgr ? R : B;
        if constexpr (D == 4) code[px][3] = to_code(rs[2], s.up);
        cv[px] = (unsigned)(fy * s.up);
    }
    if (n == kChunk && o.int_vec) {                          // (dc is a multiple of 4: the words are aligned with base and pitch)
        if constexpr (PLANAR) {
#pragma unroll
            for (int k = 0; k < D; ++k) {
                unsigned wd[BPS] = {};
#pragma unroll
                for (int px = 0; px < (int)kChunk; ++px) put_sample<BPS>(wd, px, code[px][k]);
                unsigned* q = reinterpret_cast<unsigned*>((uintptr_t)o.plane[k] + dr * o.pitch[k] + dc * BPS);
#pragma unroll
                for (int t = 0; t < BPS; ++t) q[t] = wd[t];
            }
        } else {
            unsigned wd[D * BPS] = {};
#pragma unroll
            for (int px = 0; px < (int)kChunk; ++px)
#pragma unroll
                for (int k = 0; k < D; ++k) put_sample<BPS>(wd, px * D + k, code[px][k]);
            unsigned* q = reinterpret_cast<unsigned*>((uintptr_t)o.plane[0] + dr * o.pitch[0] + dc * D * BPS);
#pragma unroll
            for (int t = 0; t < D * BPS; ++t) q[t] = wd[t];
        }
    } else {
#pragma unroll
        for (int px = 0; px < (int)kChunk; ++px)
#pragma unroll
            for (int k = 0; k < D; ++k)
                if ((unsigned)px < n) {
                    unsigned char* q = PLANAR ? reinterpret_cast<unsigned char*>((uintptr_t)o.plane[k]) + dr * o.pitch[k] + (dc + px) * BPS
                                              : reinterpret_cast<unsigned char*>((uintptr_t)o.plane[0]) + dr * o.pitch[0] + ((dc + px) * D + k) * BPS;
                    store_scalar<BPS>(q, code[px][k]);
                }
    }
    if (o.conv) {
        unsigned char* q = reinterpret_cast<unsigned char*>((uintptr_t)o.conv) + dr * o.conv_pitch + dc * BPS;
        if (n == kChunk && o.conv_vec) {
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

ListSource list_source(const RgbRule& f, const unsigned char* const src[4], const size_t spitch[4], unsigned w, unsigned h)
{
    ListSource s{};
    for (int k = 0; k < (f.planar ? f.ch : 1); ++k) { s.sp[k] = src[k]; s.spitch[k] = spitch[k]; }
    s.w = w; s.h = h;
    s.mask = f.mask; s.down = f.down; s.up = f.up; s.bgr = f.bgr ? 1 : 0;
    return s;
}

}  // namespace

void launch_rgb_list_resample(const RgbRule& f, const unsigned char* const src[4], const size_t spitch[4], unsigned w, unsigned h,
                              const DevAxisTable& th, const DevAxisTable& tv, const ListCellDesc* d, unsigned ncells, const ListCellDesc& end,
                              float* atlas, unsigned atlas_w, hipStream_t s)
{
    if (ncells == 0 || end.rs_tile0 == 0) return;
    const ListResample a{list_source(f, src, spitch, w, h), tile_tables(th, tv), d, ncells, atlas, atlas_w};
    RGB_DISPATCH(k_rgb_list_resample, f, dim3(end.rs_tile0), s, a);
}

void launch_rgb_list_merge(const RgbRule& f, const unsigned char* const src[4], const size_t spitch[4], unsigned w, unsigned h,
                           const DevAxisTable& cth, const DevAxisTable& ctv, const ListCellDesc* d, const ListDstDesc* dd, unsigned ncells,
                           const ListCellDesc& end, const float* atlas, unsigned atlas_w, hipStream_t s)
{
    if (ncells == 0 || end.sc_tile0 == 0) return;
    const ListMerge a{list_source(f, src, spitch, w, h), tile_tables(cth, ctv), d, dd, ncells, atlas, atlas_w};
    RGB_DISPATCH(k_rgb_list_merge, f, dim3(end.sc_tile0), s, a);
}

}  // namespace srcnn
