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
// multiples of that size, else sample by sample.  The kernel's body is yuv_chroma_tile (srcnn_yuv_chroma_tile.h), which
// k_yuv_list_chroma of the rect list call (srcnn_yuv_rect_list.hip) instantiates as well.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_window_tile.h"
#include "srcnn_yuv.h"
#include "srcnn_yuv_chroma_tile.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

constexpr unsigned kChunk = kTileChunk;          // samples per thread and plane

struct WinChroma {
    ChromaTileSource src;
    ChromaTileDst dst;
};

// (the body is yuv_chroma_tile of srcnn_yuv_chroma_tile.h, shared with k_yuv_list_chroma of the rect list call)
template <int BPS, bool SEMI>
__global__ __launch_bounds__(256) void k_yuv_window_chroma(const WinChroma a)
{
    yuv_chroma_tile<BPS, SEMI>(a.src, a.dst, blockIdx.x * kTileW, blockIdx.y * kTileH);      // the tile inside the chroma rect
}

}  // namespace

void launch_yuv_window_chroma(const unsigned char* const src[2], const size_t spitch[2], unsigned cw, unsigned ch, bool semi,
                              const Yuv16Rule* f, unsigned cx0, unsigned cy0, unsigned cols, unsigned rows, const DevAxisTable& th,
                              const DevAxisTable& tv, unsigned char* const dst[2], const size_t dpitch[2], hipStream_t s)
{
    if (cols == 0 || rows == 0) return;
    WinChroma a{};
    const size_t chunk = (size_t)kChunk * (f ? 2 : 1) * (semi ? 2 : 1);      // bytes of a thread's store
    a.dst.dst_vec = 1;
    for (int k = 0; k < (semi ? 1 : 2); ++k) {
        a.src.sp[k] = src[k]; a.src.spitch[k] = spitch[k];
        a.dst.dp[k] = dst[k]; a.dst.dpitch[k] = dpitch[k];
        a.dst.dst_vec = a.dst.dst_vec && aligned_to(dst[k], chunk) && dpitch[k] % chunk == 0;
    }
    a.dst.cx0 = cx0; a.dst.cy0 = cy0; a.dst.cols = cols; a.dst.rows = rows; a.src.w = cw; a.src.h = ch;
    a.src.t = tile_tables(th, tv);
    a.src.rshift = f ? f->rshift : 0; a.src.mask = f ? f->mask : 0xffu; a.src.lshift = f ? f->lshift : 0;
    a.src.maxv = f ? (float)f->mask : 255.f;
    const dim3 grid((cols + kTileW - 1) / kTileW, (rows + kTileH - 1) / kTileH);
    switch ((f ? 2 : 0) | (semi ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((k_yuv_window_chroma<1, false>), grid, dim3(256), 0, s, a); break;
    case 1: hipLaunchKernelGGL((k_yuv_window_chroma<1, true>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_yuv_window_chroma<2, false>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((k_yuv_window_chroma<2, true>), grid, dim3(256), 0, s, a); break;
    }
}

}  // namespace srcnn
