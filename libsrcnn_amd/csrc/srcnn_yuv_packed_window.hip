// srcnn_yuv_packed_window.hip -- the conversions of the packed YUV rect call (include/srcnn_amd_yuv_packed_rect.h) over a WINDOW
// of the frame: what k_yuvp_unpack -> the plane resamplers -> k_yuvp_pack (srcnn_yuv_packed.hip) do for whole rows of whole
// frames, at the cost of the rect and without a float chroma or alpha plane.
//
//   k_yuvp_window_y       a range of luma columns and rows of the packed source -> a tight float32 Y window (the source of the
//                         window Y path, y_path_rect): (float)field * 2^-s, the read rule of k_yuvp_unpack, nothing else stored
//                         -- the Y path needs the 6-sample halo, chroma does not.  One lane owns one 16-byte chunk, as there.
//   k_yuvp_window_merge   one launch per band: U', V' (and A') of one tile of the CHROMA grid of the rect resampled straight from
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
    const unsigned char* src;                    // the WHOLE frame
    size_t spitch;
    unsigned char* dst;                          // the rect's first byte
    size_t dpitch;
    const float* y;                              // Y' of the band: tight, rw floats per row
    unsigned cx0, gy0;                           // chroma output column of the rect's first column, output row of the band's first row
    unsigned row0;                               // row of the rect at which the band starts
    unsigned rw, ccols, rows;                    // luma and chroma columns of the rect, rows of the band
    unsigned cw, h;                              // source size on the chroma grid
    unsigned groups;                             // v210: 16-byte groups of a row segment, the padding groups included
    unsigned blo, bhi;                           // bytes of a source row that may be read
    TileTables t;                                // horizontal table (dcw <- cw), vertical table (dh <- h)
    YuvPackedRule f;
    int sio, dio;
};

// the dwords of chunk `c` of a row that lie inside [blo, bhi); the others stay zero
__device__ __forceinline__ void load_chunk(const unsigned char* row, unsigned c, unsigned blo, unsigned bhi, int io, unsigned q[4])
{
    const unsigned b = 16 * c;
    if (io == kIoVec && b >= blo && b + 16 <= bhi) {
        const uint4 x = *reinterpret_cast<const uint4*>(row + b);
        q[0] = x.x; q[1] = x.y; q[2] = x.z; q[3] = x.w;
    } else {
        const int piece = io == kIoVec ? kIoDword : io;
#pragma unroll
        for (unsigned j = 0; j < 4; ++j) {
            q[j] = 0;
            if (b + 4 * j >= blo && b + 4 * j + 4 <= bhi) q[j] = load_dword(row + b + 4 * j, piece);
        }
    }
}

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

// what an item of k_yuvp_window_merge is
template <int K> struct PkItem {
    using S = PkShape<K>;
    static constexpr bool V210 = K == kPkV210;
    static constexpr unsigned CPI = V210 ? 3 : kTileChunk;           // chroma samples of an item
    static constexpr unsigned STEP = S::NY / S::NC;                  // luma samples per chroma sample
    static constexpr unsigned YPI = CPI * STEP;                      // luma samples of an item
    static constexpr unsigned CHUNKS = CPI / S::NC;                  // 16-byte chunks of an item
    static constexpr unsigned TILE = V210 ? 60 : (unsigned)kTileW;   // chroma columns of a tile
    static constexpr unsigned IPR = TILE / CPI;                      // items of a tile's row
    static constexpr int NP = S::NA ? 3 : 2;                         // planes the tile resampler carries
};

template <int K>
__global__ __launch_bounds__(256) void k_yuvp_window_merge(const PkWinMerge a)
{
    using S = PkShape<K>;
    using I = PkItem<K>;
    constexpr int NP = I::NP;
    __shared__ float s_patch[NP][kPatchH][kPatchW];
    __shared__ float s_mid[NP][kTileH][kPatchW];
    __shared__ int s_span[4];
    const int tid = (int)threadIdx.x;
    const unsigned tx = blockIdx.x * I::TILE, ty = blockIdx.y * kTileH;      // the tile inside the band, on the chroma grid
    const int ncol = (int)min(I::TILE, a.ccols - tx), nrow = (int)min((unsigned)kTileH, a.rows - ty);
    const unsigned gx = a.cx0 + tx, gy = a.gy0 + ty;                         // the tile inside the dcw x dh chroma output

    // 1. - 3. (srcnn_window_tile.h); a staged sample is U, V (and A) of a source chroma column: the fields of its chunk
    const TilePatch p = tile_patch(a.t, s_span, tid, gx, gy, ncol, nrow, a.cw, a.h);
    tile_stage<NP>(s_patch, p, tid, [&](size_t sr, size_t sc, float* out) {
        const unsigned c = (unsigned)sc / S::NC, k = (unsigned)sc % S::NC;
        unsigned q[4];
        load_chunk(a.src + sr * a.spitch, c, a.blo, a.bhi, a.sio, q);
        unsigned y[8], u[4], v[4], al[4] = {0, 0, 0, 0};
        decode<K>(q, a.f, y, u, v, al);
        unsigned su = 0, sv = 0, sa = 0;
#pragma unroll
        for (unsigned j = 0; j < S::NC; ++j) {
            su = j == k ? u[j] : su;
            sv = j == k ? v[j] : sv;
            if constexpr (S::NA > 0) sa = j == k ? al[j] : sa;
        }
        out[0] = (float)su;
        out[1] = (float)sv;
        if constexpr (S::NA > 0) out[2] = (float)sa;
    });
    __syncthreads();
    tile_vertical<NP>(a.t, s_patch, s_mid, p, tid, gy, nrow);
    __syncthreads();

    // 4. horizontal pass, saturate, merge with Y', encode, store: one item at a time.  v210: the last tile of a row of tiles also
    // owns the groups that only pad the row segment.
    const float maxv = (float)a.f.mask, amax = (float)a.f.amask;
    unsigned ipr = I::IPR;
    if constexpr (I::V210)
        if (blockIdx.x == gridDim.x - 1) ipr = a.groups - blockIdx.x * I::IPR;
    const unsigned items = (unsigned)nrow * ipr;
    for (unsigned it = (unsigned)tid; it < items; it += kTileThreads) {
        const unsigned ry = it / ipr, c = (it - ry * ipr) * I::CPI;          // row and first chroma column inside the tile
        const unsigned n = c < (unsigned)ncol ? min(I::CPI, (unsigned)ncol - c) : 0u;    // chroma samples of the item
        if (!I::V210 && n == 0) continue;
        const size_t br = (size_t)ty + ry;                       // row of the band
        const size_t dr = (size_t)a.row0 + br;                   // row of the rect = destination row
        const unsigned dc = tx + c;                              // chroma column of the rect
        const unsigned y0 = I::STEP * dc;                        // luma column of the rect
        const unsigned ny = y0 < a.rw ? min(I::YPI, a.rw - y0) : 0u;
        unsigned y[I::YPI], u[I::CPI], v[I::CPI], al[I::CPI];
#pragma unroll
        for (unsigned k = 0; k < I::CPI; ++k) {
            float rs[3] = {0.f, 0.f, 0.f};
            if (k < n) tile_horizontal<NP>(a.t, s_mid, p, (int)ry, gx + c + k, rs);
            u[k] = k < n ? to_word<true>(rs[0], 1.f, maxv) : 0u;
            v[k] = k < n ? to_word<true>(rs[1], 1.f, maxv) : 0u;
            al[k] = (S::NA > 0 && k < n) ? to_word<true>(rs[2], 1.f, amax) : 0u;
        }
#pragma unroll
        for (unsigned k = 0; k < I::YPI; ++k) {
            float fy = 0.f;
            if (k < ny) fy = a.y[br * a.rw + y0 + k];
            y[k] = k < ny ? to_word<false>(fy, a.f.up, maxv) : 0u;
        }
        unsigned q[4 * I::CHUNKS];
#pragma unroll
        for (unsigned j = 0; j < I::CHUNKS; ++j) encode<K>(y + j * S::NY, u + j * S::NC, v + j * S::NC, al + j * S::NC, a.f, q + 4 * j);
        // dwords of the item that belong to the span: a chroma sample of the 4:2:2 and 4:4:4 kinds is 1 or 2 dwords; v210: the group
        const unsigned nd = I::V210 ? 4u : n * (4 * I::CHUNKS / I::CPI);
        unsigned char* d = a.dst + dr * a.dpitch + (size_t)(dc / I::CPI) * (16 * I::CHUNKS);
        if (nd == 4 * I::CHUNKS && a.dio == kIoVec) {
#pragma unroll
            for (unsigned j = 0; j < I::CHUNKS; ++j)
                *reinterpret_cast<uint4*>(d + 16 * j) = make_uint4(q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]);
        } else {
            const int piece = a.dio == kIoVec ? kIoDword : a.dio;
#pragma unroll
            for (unsigned j = 0; j < 4 * I::CHUNKS; ++j)
                if (j < nd) store_dword(d + 4 * j, q[j], piece);
        }
    }
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

// bytes [blo, bhi) of a row of the w-pixel frame that hold luma columns [lx, hx) widened to the unit
void span_of(int kind, unsigned w, unsigned lx, unsigned hx, unsigned& blo, unsigned& bhi)
{
    const unsigned unit = yuv_packed_unit(kind);
    lx -= lx % unit;
    hx = std::min(w, (hx + unit - 1) / unit * unit);
    size_t off = 0, n = 0;
    yuv_packed_span(kind, w, lx, hx - lx, off, n);
    blo = (unsigned)off;
    bhi = (unsigned)(off + n);
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
    span_of(f.kind, w, sx0, sx0 + sw, a.blo, a.bhi);
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
    a.src = src; a.spitch = spitch; a.dst = dst; a.dpitch = dpitch; a.y = yband;
    a.cx0 = cx0; a.gy0 = gy0; a.row0 = row0; a.rw = rw; a.ccols = ccols; a.rows = rows;
    a.cw = yuv_packed_chroma_cols(f.kind, w); a.h = h;
    a.groups = (unsigned)(span_bytes / 16);
    a.blo = 0; a.bhi = (unsigned)yuv_packed_row_bytes(f.kind, w);
    // the source columns the taps of the rect's chroma columns read, as luma columns (the tables have host copies: the caller asked
    // yuvp_window_fits)
    if (th.h_first && th.h_taps) {
        int lo = 0x7fffffff, hi = 0;
        for (unsigned x = cx0; x < cx0 + ccols; ++x) { lo = std::min(lo, th.h_first[x]); hi = std::max(hi, th.h_first[x] + th.h_taps[x]); }
        const unsigned step = yuv_packed_chroma_step(f.kind);
        span_of(f.kind, w, (unsigned)std::max(lo, 0) * step, std::min((unsigned)hi * step, w), a.blo, a.bhi);
    }
    a.t = tile_tables(th, tv);
    a.f = f;
    a.sio = io_of(src, spitch);
    a.dio = io_of(dst, dpitch);
    const unsigned tile = yuv_packed_tile_cols(f.kind);
    const dim3 grid((ccols + tile - 1) / tile, (rows + kTileH - 1) / kTileH), b(kTileThreads);
#define SRCNN_YUVP_WINDOW_MERGE(K) hipLaunchKernelGGL(k_yuvp_window_merge<K>, grid, b, 0, s, a)
    SRCNN_YUVP_KINDS(SRCNN_YUVP_WINDOW_MERGE, f.kind)
#undef SRCNN_YUVP_WINDOW_MERGE
}

}  // namespace srcnn
