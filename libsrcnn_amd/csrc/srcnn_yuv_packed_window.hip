// srcnn_yuv_packed_window.hip -- the conversions of the packed YUV rect call (include/srcnn_amd_yuv_packed_rect.h) over a WINDOW
// of the frame: what k_yuvp_unpack -> the plane resamplers -> k_yuvp_pack (srcnn_yuv_packed.hip) do for whole rows of whole
// frames, at the cost of the rect and without a float chroma or alpha plane.
//
//   k_yuvp_window_y       a range of luma columns and rows of the packed source -> a tight float32 Y window (the source of the
//                         window Y path, y_path_rect): (float)field * 2^-s, the read rule of k_yuvp_unpack, nothing else stored
//                         -- the Y path needs the 6-sample halo, chroma does not.  One lane owns one 16-byte chunk, as there.
//   k_yuvp_window_merge   (its body is yuvp_merge_tile of srcnn_yuv_packed_merge_tile.h, which the packed rect LIST call's
//                         k_yuvp_list_merge instantiates too; what follows describes that body)
//                         one launch per band: U', V' (and A') of one tile of the CHROMA grid of the rect resampled straight from
//                         the packed integer source (the tile resampler, srcnn_window_tile.h, which describes its four steps and
//                         says which shapes it serves; the staged sample is decoded by decode<K>), saturated, put beside the
//                         finished Y' of the band, converted as k_yuvp_pack converts them, encoded by encode<K> and stored.
//
// The layouts are srcnn_yuv_packed_fields.h and the pixel rules srcnn_colour_rules.h, both shared with srcnn_yuv_packed.hip.
//
// Tiles and items.  A workgroup of 256 threads takes 64 x 16 samples of the chroma grid -- 128 x 16 luma samples for the 4:2:2
// kinds, 64 x 16 for 4:4:4 + alpha.  An item is 4 consecutive chroma samples of one row with the luma samples beside them (8 or
// 4): one 16-byte chunk of YUY2 / VUYA / Y410, two of Y21x / Y416; a tile has 16 x 16 items, one per thread.
// v210 packs 3 chroma samples per 16-byte group, which divides neither 64 nor 4.  Of the two ways out this file takes the NARROWER
// TILE: 60 chroma columns, 20 groups, item = group (3 chroma, 6 luma samples, one chunk); the 16 x 20 items of a tile are dealt
// over the 256 threads in a loop, and the host asks the route predicate with that width (yuvp_window_fits).  The float results
// are the tile resampler's, unchanged; no group is written by two threads.  Where a v210 rect reaches the right border its span
// runs to the end of the row's last 128-byte block: the groups that only pad the row belong to the last tile of each row of
// tiles, as items without a sample, and are written as zero.
//
// Stores.  An item goes out as one 16-byte store per chunk where the destination's base and pitch are multiples of 16 (the
// rect's first byte is an item boundary, and so is every item's); otherwise, and for the partial item at the right border, dword
// by dword in pieces of the alignment the frame has -- io_of, as in k_yuvp_pack.  A thread stores only bytes of the rect's span,
// the zero slots the span includes at the right border among them, and never reads the destination.
//
// Reads.  Every access to the source is a dword inside a byte range of the row that the host derives from the source rectangle
// the call reports (yuv_packed_span): a dword of a chunk outside it is not loaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_window_tile.h"
#include "srcnn_yuv.h"
#include "srcnn_yuv_packed_fields.h"
#include "srcnn_yuv_packed_merge_tile.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

struct PkWinY {
    const unsigned char* src;                    // the WHOLE frame
    size_t pitch;
    float* y;                                    // tight, sw floats per row
    unsigned sx0, sy0, sw, rows;                 // the window in luma samples
    unsigned c0, cpr;                            // first chunk of a row that holds a sample of the window, chunks per row
    unsigned blo, bhi;                           // bytes of a row that may be read
    YuvPackedRule f;
    int io;
};

struct PkWinMerge {
    PkMergeSource s;
    PkMergeRect r;                               // one band of the rect: r.y is tight, rw floats per row
};

template <int K>
__global__ __launch_bounds__(256) void k_yuvp_window_y(const PkWinY a)
{
    using S = PkShape<K>;
    const unsigned total = a.cpr * a.rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / a.cpr, c = a.c0 + (i - r * a.cpr);
        unsigned q[4];
        load_chunk(a.src + (size_t)(a.sy0 + r) * a.pitch, c, a.blo, a.bhi, a.io, q);
        unsigned y[8], u[4], v[4], al[4];
        decode<K>(q, a.f, y, u, v, al);
        float* d = a.y + (size_t)r * a.sw;
#pragma unroll
        for (unsigned k = 0; k < S::NY; ++k) {
            const unsigned col = S::NY * c + k;
            if (col >= a.sx0 && col - a.sx0 < a.sw) d[col - a.sx0] = (float)y[k] * a.f.down;
        }
    }
}

// one workgroup per tile of the band's chroma grid: the body is yuvp_merge_tile (srcnn_yuv_packed_merge_tile.h)
template <int K>
__global__ __launch_bounds__(256) void k_yuvp_window_merge(const PkWinMerge a)
{
    yuvp_merge_tile<K>(a.s, a.r, blockIdx.x, blockIdx.y, blockIdx.x == gridDim.x - 1);
}

#define SRCNN_YUVP_KINDS(X, kind) \
    switch (kind) {               \
    case kPk422x8: X(kPk422x8); break;   \
    case kPk422x16: X(kPk422x16); break; \
    case kPk444x8: X(kPk444x8); break;   \
    case kPk410: X(kPk410); break;       \
    case kPk444x16: X(kPk444x16); break; \
    default: X(kPkV210); break;          \
    }

unsigned chunk_luma(int kind)
{
    switch (kind) {
    case kPk422x8: return 8;
    case kPk444x16: return 2;
    case kPkV210: return 6;
    default: return 4;
    }
}

}  // namespace

void launch_yuvp_window_y(const YuvPackedRule& f, const unsigned char* src, size_t pitch, unsigned w, unsigned sx0, unsigned sy0, unsigned sw,
                          unsigned sh, float* y, hipStream_t s)
{
    if (sw == 0 || sh == 0) return;
    PkWinY a{};
    const unsigned ny = chunk_luma(f.kind);
    a.src = src; a.pitch = pitch; a.y = y;
    a.sx0 = sx0; a.sy0 = sy0; a.sw = sw; a.rows = sh;
    a.c0 = sx0 / ny;
    a.cpr = (sx0 + sw + ny - 1) / ny - a.c0;
    yuv_packed_unit_span(f.kind, w, sx0, sx0 + sw, a.blo, a.bhi);
    a.f = f;
    a.io = io_of(src, pitch);
    const dim3 g = grid_for((size_t)a.cpr * sh, 4096), b(256);
#define SRCNN_YUVP_WINDOW_Y(K) hipLaunchKernelGGL(k_yuvp_window_y<K>, g, b, 0, s, a)
    SRCNN_YUVP_KINDS(SRCNN_YUVP_WINDOW_Y, f.kind)
#undef SRCNN_YUVP_WINDOW_Y
}

void launch_yuvp_window_merge(const YuvPackedRule& f, const unsigned char* src, size_t spitch, unsigned w, unsigned h, const float* yband,
                              unsigned cx0, unsigned gy0, unsigned rw, unsigned ccols, unsigned rows, const DevAxisTable& th,
                              const DevAxisTable& tv, unsigned char* dst, size_t dpitch, unsigned row0, size_t span_bytes, hipStream_t s)
{
    if (rw == 0 || ccols == 0 || rows == 0) return;
    PkWinMerge a{};
    a.s.src = src; a.s.spitch = spitch; a.r.dst = dst; a.r.dpitch = dpitch; a.r.y = yband; a.r.ystride = rw;
    a.r.cx0 = cx0; a.r.gy0 = gy0; a.r.row0 = row0; a.r.rw = rw; a.r.ccols = ccols; a.r.rows = rows;
    a.s.cw = yuv_packed_chroma_cols(f.kind, w); a.s.h = h;
    a.r.groups = (unsigned)(span_bytes / 16);
    a.r.blo = 0; a.r.bhi = (unsigned)yuv_packed_row_bytes(f.kind, w);
    // the source columns the taps of the rect's chroma columns read, as luma columns (the tables have host copies: the caller asked
    // yuvp_window_fits)
    if (th.h_first && th.h_taps) {
        int lo = 0x7fffffff, hi = 0;
        for (unsigned x = cx0; x < cx0 + ccols; ++x) { lo = std::min(lo, th.h_first[x]); hi = std::max(hi, th.h_first[x] + th.h_taps[x]); }
        const unsigned step = yuv_packed_chroma_step(f.kind);
        yuv_packed_unit_span(f.kind, w, (unsigned)std::max(lo, 0) * step, std::min((unsigned)hi * step, w), a.r.blo, a.r.bhi);
    }
    a.s.t = tile_tables(th, tv);
    a.s.f = f;
    a.s.sio = io_of(src, spitch);
    a.r.dio = io_of(dst, dpitch);
    const unsigned tile = yuv_packed_tile_cols(f.kind);
    const dim3 grid((ccols + tile - 1) / tile, (rows + kTileH - 1) / kTileH), b(kTileThreads);
#define SRCNN_YUVP_WINDOW_MERGE(K) hipLaunchKernelGGL(k_yuvp_window_merge<K>, grid, b, 0, s, a)
    SRCNN_YUVP_KINDS(SRCNN_YUVP_WINDOW_MERGE, f.kind)
#undef SRCNN_YUVP_WINDOW_MERGE
}

}  // namespace srcnn
