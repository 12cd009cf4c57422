// srcnn_rect_list.hip -- the kernels of the rect LIST call (include/srcnn_amd_rect_list.h): many windows of the upscaled plane
// packed into one scratch image, the atlas, so that the unchanged layer kernels run over all of them in one launch each.
//
//   k_list_resample    the in-plane part of every cell, resampled from the source plane by the tile resampler
//                      (srcnn_window_tile.h, NC = 1 with a float fetch): the bits of the plane resamplers.  Its body is
//                      list_resample_tile of srcnn_rect_list.h, which the RGB(A) list instantiates with an integer fetch
//   k_list_replicate   the out-of-plane part of every cell that has one, within `depth` samples of the rect: the cell's own
//                      sample at the clamped coordinate.  Depth 6 on the upscaled plane (what the 9x9 layer's clamp-to-edge
//                      reads), depth 2 on the 32 layer-2 planes (layer 3 clamps the ACTIVATIONS to the edge, and layer 2 over a
//                      replicated input is not the replicated activation).  It reads in-plane samples and writes out-of-plane
//                      ones only, so no thread reads what another writes.
//   k_list_scatter     every rect from the atlas result to its own d_out and pitch
//
// One workgroup of 256 threads takes one 64 x 16 tile of one cell.  Which cell: the descriptor table (ListCellDesc,
// srcnn_rect_atlas.hpp) carries a prefix sum of tiles per kernel, and a workgroup finds the cell its index falls in by bisection
// -- the same for all its threads.  The table has one closing entry with the totals; the grids are exactly those totals.
//
// Every index is bounded: a tile is cut to its cell part, cells lie inside the atlas (tests/host/rect_list_sanitize.cpp), the
// source patch is clamped to the w x h plane (tile_patch), and a store to d_out stays inside the rect's rw floats per row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_rect_list.h"
#include "srcnn_window_tile.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr int kCols = kTileW / (int)kTileChunk;      // threads per tile row

__global__ __launch_bounds__(256) void k_list_resample(const float* __restrict__ in, size_t in_stride, unsigned w, unsigned h, const TileTables t,
                                                       const ListCellDesc* __restrict__ d, unsigned n, float* __restrict__ atlas, unsigned atlas_w)
{
    list_resample_tile(w, h, t, d, n, atlas, atlas_w, [&](size_t sr, size_t sc, float* v) { v[0] = in[sr * in_stride + sc]; });
}

__global__ __launch_bounds__(256) void k_list_replicate(const ListCellDesc* __restrict__ d, unsigned n, float* __restrict__ atlas, unsigned atlas_w,
                                                        size_t plane_stride, unsigned depth)
{
    const int tid = (int)threadIdx.x;
    const ListCellDesc c = d[find_cell<&ListCellDesc::rep_tile0>(d, n, blockIdx.x)];
    const unsigned tile = blockIdx.x - c.rep_tile0, tiles_x = (c.cw + kTileW - 1) / kTileW;
    const unsigned j = (tile / tiles_x) * kTileH + tid / kCols;                          // row of the cell
    const unsigned i0 = (tile % tiles_x) * kTileW + (tid % kCols) * kTileChunk;          // first of this thread's columns
    const unsigned lo = kCellMargin - depth;                                             // the ring: [lo, 6 + rw + depth) x [lo, 6 + rh + depth)
    if (j < lo || j >= kCellMargin + c.rh + depth || j >= c.ch) return;
    float* cell = atlas + (size_t)blockIdx.y * plane_stride + (size_t)c.ay * atlas_w + c.ax;
    const unsigned cj = min(max(j, c.oy), c.oy + c.ih - 1);
    const bool row_out = j != cj;
    for (unsigned i = i0; i < i0 + kTileChunk; ++i) {
        if (i < lo || i >= kCellMargin + c.rw + depth || i >= c.cw) continue;
        const unsigned ci = min(max(i, c.ox), c.ox + c.iw - 1);
        if (row_out || i != ci) cell[(size_t)j * atlas_w + i] = cell[(size_t)cj * atlas_w + ci];
    }
}

__global__ __launch_bounds__(256) void k_list_scatter(const ListCellDesc* __restrict__ d, unsigned n, const float* __restrict__ atlas, unsigned atlas_w)
{
    const int tid = (int)threadIdx.x;
    const ListCellDesc c = d[find_cell<&ListCellDesc::sc_tile0>(d, n, blockIdx.x)];
    const unsigned tile = blockIdx.x - c.sc_tile0, tiles_x = (c.rw + kTileW - 1) / kTileW;
    const unsigned y = (tile / tiles_x) * kTileH + tid / kCols;                          // row of the rect
    const unsigned x = (tile % tiles_x) * kTileW + (tid % kCols) * kTileChunk;           // first of this thread's columns
    if (y >= c.rh || x >= c.rw) return;
    const float* in = atlas + (size_t)(c.ay + kCellMargin + y) * atlas_w + (c.ax + kCellMargin + x);
    float* out = reinterpret_cast<float*>((uintptr_t)c.out) + (size_t)y * c.out_stride + x;
    const unsigned nn = min(kTileChunk, c.rw - x);
    if (nn == kTileChunk && c.out_vec) {                     // (x is a multiple of 4: out is 16-byte aligned with d_out)
        *reinterpret_cast<float4*>(out) = make_float4(in[0], in[1], in[2], in[3]);
    } else {
        for (unsigned k = 0; k < nn; ++k) out[k] = in[k];
    }
}

}  // namespace

void launch_list_resample(const float* d_in, size_t in_stride, unsigned w, unsigned h, const DevAxisTable& th, const DevAxisTable& tv,
                          const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas, unsigned atlas_w, hipStream_t s)
{
    if (ncells == 0 || end.rs_tile0 == 0) return;
    hipLaunchKernelGGL(k_list_resample, dim3(end.rs_tile0), dim3(kTileThreads), 0, s, d_in, in_stride, w, h, tile_tables(th, tv), d, ncells, atlas, atlas_w);
}

void launch_list_replicate(const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, float* atlas, unsigned atlas_w, size_t plane_stride,
                           unsigned planes, unsigned depth, hipStream_t s)
{
    if (ncells == 0 || end.rep_tile0 == 0 || planes == 0 || depth > kCellMargin) return;
    hipLaunchKernelGGL(k_list_replicate, dim3(end.rep_tile0, planes), dim3(kTileThreads), 0, s, d, ncells, atlas, atlas_w, plane_stride, depth);
}

void launch_list_scatter(const ListCellDesc* d, unsigned ncells, const ListCellDesc& end, const float* atlas, unsigned atlas_w, hipStream_t s)
{
    if (ncells == 0 || end.sc_tile0 == 0) return;
    hipLaunchKernelGGL(k_list_scatter, dim3(end.sc_tile0), dim3(kTileThreads), 0, s, d, ncells, atlas, atlas_w);
}

}  // namespace srcnn
