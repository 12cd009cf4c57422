// srcnn_window.hip -- the kernels of the rect call (include/srcnn_amd_rect.h): a WINDOW of the resampled plane, and the store
// of a window's interior into the caller's pitched buffer.
//
//   k_win_rows   horizontal pass (horizontalFilter, src/frawscale.cpp:338-385) for a range of destination columns
//   k_win_cols   vertical pass (verticalFilter, src/frawscale.cpp:288-336) for a range of destination rows and columns
//   k_win_copy   a w x rows block of floats between two strided buffers
//
// The two passes are k_resample_rows / k_resample_cols of srcnn_kernels.hip with a column base and strides: the same
// operations in the same order -- acc = 0.0; acc = acc + wt[t] * (double)px over the taps in table order; one (float)acc --
// so a window holds the bits the whole-plane resamplers put at the same place (this TU is built with -ffp-contract=off like
// theirs, and says so again below).  What makes them window kernels is their cost: one thread per sample of the window, a
// 64 x 4 block, so a launch scales with the window's area and never with the width or height of the plane around it.  The
// host side (resample_window in srcnn_capi.cpp) orders the passes as the reference does and sizes the intermediate image from
// the contribution tables.
//
// Every index is bounded by the launch arguments: a thread leaves when its column is outside [0, nc), rows are walked with a
// grid stride below `rows`, and the taps of a sample lie inside the span the host computed from the same table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "srcnn_window.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr int WIN_BX = 64, WIN_BY = 4;       // block: one wave per row, four rows

__global__ __launch_bounds__(WIN_BX * WIN_BY) void k_win_rows(
    const float* __restrict__ src, size_t src_stride, int src_col_base, float* __restrict__ dst, int c0, int nc, int rows,
    const int* __restrict__ first, const int* __restrict__ taps, const double* __restrict__ wt, int stride)
{
    const int xi = blockIdx.x * WIN_BX + threadIdx.x;
    if (xi >= nc) return;
    const int x = c0 + xi;
    const int s0 = first[x] - src_col_base, n = taps[x];
    const double* wr = wt + (size_t)x * stride;
    for (int y = blockIdx.y * WIN_BY + threadIdx.y; y < rows; y += gridDim.y * WIN_BY) {
        const float* in = src + (size_t)y * src_stride + s0;
        double acc = 0.0;
        for (int t = 0; t < n; ++t) acc = acc + wr[t] * (double)in[t];
        dst[(size_t)y * nc + xi] = (float)acc;
    }
}

__global__ __launch_bounds__(WIN_BX * WIN_BY) void k_win_cols(
    const float* __restrict__ src, size_t src_stride, int src_row_base, float* __restrict__ dst, int nc, int r0, int rows,
    const int* __restrict__ first, const int* __restrict__ taps, const double* __restrict__ wt, int stride)
{
    const int xi = blockIdx.x * WIN_BX + threadIdx.x;
    if (xi >= nc) return;
    for (int ry = blockIdx.y * WIN_BY + threadIdx.y; ry < rows; ry += gridDim.y * WIN_BY) {
        const int y = r0 + ry;
        const int s0 = first[y] - src_row_base, n = taps[y];
        const double* wr = wt + (size_t)y * stride;
        double acc = 0.0;
        for (int t = 0; t < n; ++t) {
            const double px = (double)src[(size_t)(s0 + t) * src_stride + xi];
            acc = acc + wr[t] * px;
        }
        dst[(size_t)ry * nc + xi] = (float)acc;
    }
}

// A row is `head` single floats up to the first 16-byte boundary of the destination, nvec 16-byte units, and the single
// floats that are left: thread u < nvec stores unit u (its four floats are loaded one by one: the source window starts
// wherever the halo puts it), the threads after them one float each.  nvec == 0: all single floats.
__global__ __launch_bounds__(WIN_BX * WIN_BY) void k_win_copy(
    const float* __restrict__ src, size_t src_stride, float* __restrict__ dst, size_t dst_stride, int w, int rows, int head, int nvec)
{
    const int u = blockIdx.x * WIN_BX + threadIdx.x;
    if (u >= nvec + (w - 4 * nvec)) return;
    for (int y = blockIdx.y * WIN_BY + threadIdx.y; y < rows; y += gridDim.y * WIN_BY) {
        const float* in = src + (size_t)y * src_stride;
        float* out = dst + (size_t)y * dst_stride;
        if (u < nvec) {
            const int c = head + 4 * u;
            const float4 v = make_float4(in[c], in[c + 1], in[c + 2], in[c + 3]);
            *reinterpret_cast<float4*>(out + c) = v;
        } else {
            const int k = u - nvec;
            const int c = k < head ? k : 4 * nvec + k;
            out[c] = in[c];
        }
    }
}

dim3 win_grid(int units, int rows)
{
    return dim3((unsigned)((units + WIN_BX - 1) / WIN_BX), (unsigned)std::min((rows + WIN_BY - 1) / WIN_BY, 65535));
}

}  // namespace

void launch_window_rows(const float* src, size_t src_stride, int src_col_base, float* dst, int c0, int nc, int rows,
                        const DevAxisTable& t, hipStream_t s)
{
    if (nc <= 0 || rows <= 0) return;
    hipLaunchKernelGGL(k_win_rows, win_grid(nc, rows), dim3(WIN_BX, WIN_BY), 0, s, src, src_stride, src_col_base, dst, c0, nc, rows,
                       t.first, t.taps, t.weight, t.stride);
}

void launch_window_cols(const float* src, size_t src_stride, int src_row_base, float* dst, int nc, int r0, int rows,
                        const DevAxisTable& t, hipStream_t s)
{
    if (nc <= 0 || rows <= 0) return;
    hipLaunchKernelGGL(k_win_cols, win_grid(nc, rows), dim3(WIN_BX, WIN_BY), 0, s, src, src_stride, src_row_base, dst, nc, r0, rows,
                       t.first, t.taps, t.weight, t.stride);
}

void launch_window_copy(const float* src, size_t src_stride, float* dst, size_t dst_stride, int w, int rows, hipStream_t s)
{
    if (w <= 0 || rows <= 0) return;
    int head = 0, nvec = 0;
    if (dst_stride % 4 == 0 || rows == 1) {        // every row of dst then starts at the same offset from a 16-byte boundary
        head = std::min(w, (int)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / sizeof(float)));
        nvec = (w - head) / 4;
        if (nvec == 0) head = 0;
    }
    hipLaunchKernelGGL(k_win_copy, win_grid(nvec + (w - 4 * nvec), rows), dim3(WIN_BX, WIN_BY), 0, s, src, src_stride, dst, dst_stride,
                       w, rows, head, nvec);
}

}  // namespace srcnn
