// fake_kernels_tiers.cpp -- launch_conv12_tiers on the fake HIP runtime.
//
// k_conv12_tiers reads and writes exactly what the strict LDS-DMA instance of k_conv12_mfma does (same grid, tile queue, clock
// slot, planes), and computes the same bits, so its CPU closure is that launcher's (fake_kernels.cpp): same declared footprint,
// same queue check, same arithmetic.  run_layer12 (srcnn_capi.cpp) reaches this entry for every strict call of the harness.
#include "../../libsrcnn_amd/csrc/srcnn_window.h"

namespace srcnn {

void launch_conv12_tiers(const float* Y, int W, int H, int y_row_base, int y_rows, float* C2, size_t plane_stride, int out_row0,
                         int out_rows, int num_cus, hipStream_t s, unsigned long long* clk, unsigned* queue)
{
    launch_conv12_mfma(Y, W, H, y_row_base, y_rows, C2, plane_stride, out_row0, out_rows, 0, num_cus, s, clk, queue);
}

}  // namespace srcnn
