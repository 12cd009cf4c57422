// srcnn_rect_list.h -- launchers of the rect list call's kernels (srcnn_rect_list.hip), for srcnn_capi.cpp, and the device code
// those kernels share with the RGB(A) list's (srcnn_rgb_rect_list.hip), the YUV list's (srcnn_yuv_rect_list.hip) and the packed
// YUV list's (srcnn_yuv_packed_rect_list.hip).  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "srcnn_kernels.h"
#include "srcnn_rect_atlas.hpp"
#include "srcnn_window_tile.h"

namespace srcnn {

// d: the device copy of a pass's descriptor table (ncells + 1 entries, build_cell_descs); `end`: its closing entry (the totals).
// atlas_w: floats per row of the atlas planes.
void launch_list_resample(const float* d_in, size_t in_stride, unsigned w, unsigned h, const DevAxisTable& th, const DevAxisTable& tv,
                          const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas, unsigned atlas_w, hipStream_t s);
// out-of-plane samples within `depth` of the rect, in `planes` planes `plane_stride` floats apart
void launch_list_replicate(const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas, unsigned atlas_w, size_t plane_stride,
                           unsigned planes, unsigned depth, hipStream_t s);
void launch_list_scatter(const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, const float* atlas, unsigned atlas_w, hipStream_t s);

#ifdef __HIPCC__
#pragma clang fp contract(off)

// the largest k < n with d[k].*START <= b (d[0].*START == 0, and b is below the total)
template <unsigned ListCellDesc::*START>
__device__ __forceinline__ unsigned find_cell(const ListCellDesc* __restrict__ d, unsigned n, unsigned b)
{
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (d[mid].*START <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// The body of the resample kernels of all four lists: workgroup blockIdx.x takes one 64 x 16 tile of the in-plane part of one cell
// and writes its samples of the upscaled plane into the atlas.  fetch(source row, source column, float v[1]) gives a source
// sample of the w x h plane as a float: the one part that belongs to the caller's format.  Every return ahead of a barrier
// depends on the cell and the tile alone, which are the same for all threads of the workgroup.
template <class Fetch>
__device__ __forceinline__ void list_resample_tile(unsigned w, unsigned h, const TileTables& t, const ListCellDesc* __restrict__ d, unsigned n,
                                                   float* __restrict__ atlas, unsigned atlas_w, Fetch fetch)
{
    constexpr int kCols = kTileW / (int)kTileChunk;      // threads per tile row
    __shared__ float s_patch[1][kPatchH][kPatchW];
    __shared__ float s_mid[1][kTileH][kPatchW];
    __shared__ int s_span[4];
    const int tid = (int)threadIdx.x;
    const ListCellDesc c = d[find_cell<&ListCellDesc::rs_tile0>(d, n, blockIdx.x)];
    const unsigned tile = blockIdx.x - c.rs_tile0, tiles_x = (c.iw + kTileW - 1) / kTileW;
    const unsigned tx = (tile % tiles_x) * kTileW, ty = (tile / tiles_x) * kTileH;       // the tile inside the in-plane part
    if (tx >= c.iw || ty >= c.ih) return;                                                // (never: the prefix sums count these tiles)
    const int ncol = (int)min((unsigned)kTileW, c.iw - tx), nrow = (int)min((unsigned)kTileH, c.ih - ty);
    const unsigned gx = c.px + tx, gy = c.py + ty;                                       // the tile on the dw x dh plane

    const TilePatch p = tile_patch(t, s_span, tid, gx, gy, ncol, nrow, w, h);
    if (p.pw <= 0 || p.ph <= 0) return;                                                  // (never: window_tile_fits)
    tile_stage<1>(s_patch, p, tid, fetch);
    __syncthreads();
    tile_vertical<1>(t, s_patch, s_mid, p, tid, gy, nrow);
    __syncthreads();

    const int ry = tid / kCols, cc = (tid % kCols) * (int)kTileChunk;
    if (ry >= nrow || cc >= ncol) return;
    const int nn = min((int)kTileChunk, ncol - cc);
    float* out = atlas + (size_t)(c.ay + c.oy + ty + ry) * atlas_w + (c.ax + c.ox + tx + cc);
    for (int px = 0; px < nn; ++px) {
        float rs[1] = {0.f};
        tile_horizontal<1>(t, s_mid, p, ry, gx + cc + px, rs);
        out[px] = rs[0];
    }
}
#endif  // __HIPCC__

}  // namespace srcnn
