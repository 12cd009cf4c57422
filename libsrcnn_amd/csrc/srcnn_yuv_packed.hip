// srcnn_yuv_packed.hip -- the conversions around the SRCNN path for PACKED YUV frames (include/srcnn_amd_yuv_packed.h): one
// plane whose rows interleave Y, U, V and, for the 4:4:4 formats, alpha.
//
//   k_yuvp_unpack   pitched packed rows -> tight float32 planes Y, U, V (A)
//                   Y = (float)field * 2^-s; U, V, A = (float)field (all exact in fp32).  Only the bits of a field are read.
//   k_yuvp_pack     tight float32 rows Y' (one band), U', V' (A') (the same rows of the finished planes) -> pitched packed rows
//                   Y':         (unsigned) (v * 2^s)              layer 3 already clamps v to [0, 255]
//                   U', V', A': MIN(maxv), MAX(0), truncation      the reference's macro forms on the native scale
//                   every byte of the tight rows is written once; slots that carry no sample are written as zero
//
// Six memory layouts (YuvPackedKind) carry the ten public formats, each stated once in srcnn_yuv_packed_fields.h (shared with
// the window kernels of srcnn_yuv_packed_window.hip); byte positions, shift, maxv and scale are kernel arguments.  Both kernels are memory-bound.  One lane owns one 16-byte chunk of a packed row -- 8 YUY2 pixels, 4 Y210 /
// VUYA / Y410 pixels, 2 Y416 pixels or one v210 group of 6 -- and consecutive lanes own consecutive chunks, so a wave reads
// or writes 1 KiB of packed data in one instruction where base and pitch are 16-byte aligned (decided once per launch).
// Misaligned frames and a row's last partial chunk move their dwords one by one, in pieces of the alignment the frame has
// (4, 2 or 1 bytes).  The float side uses float4 / float2 where the row length keeps every row start aligned for it (again
// once per launch), else scalars.
//
// v210: a group's 6 luma floats start at 24 * group bytes, which no float4 store can take at every group.  The mapping stays
// lane = group: a lane moves its 6 Y as three float2 (8-byte aligned whenever w is even) and its 3 + 3 chroma as dwords.
// The 64 lanes of a wave then cover ONE contiguous span of 1536 B of Y and 768 B of each chroma plane, so every cache
// line of the planes is still written in full by one instruction group; giving a lane two groups for float4 stores would
// stride the packed side by 32 B instead and halve the 16-byte coalescing there.  In the pack kernel the groups that only
// pad a row to its 128-byte block are chunks like any other, with no valid sample: they are written as zero.
//
// Grid-stride over rows x chunks.  The host side is srcnn_frames.cpp (yuv_packed_frame); planar and semi-planar frames are
// srcnn_yuv_planes.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "srcnn_colour_rules.h"
#include "srcnn_pixel_io.h"
#include "srcnn_yuv.h"
#include "srcnn_yuv_packed_fields.h"

#pragma clang fp contract(off)

namespace srcnn {

namespace {

__device__ __forceinline__ unsigned valid_of(unsigned per_chunk, unsigned chunk, unsigned have)
{
    const unsigned first = per_chunk * chunk;
    return first >= have ? 0u : min(per_chunk, have - first);
}

// cpr: 16-byte chunks of a row that carry a sample; row_dwords: dwords of a tight row; cw: chroma samples of a row.
// io: kIo* of the packed side; fvec: vector accesses on the float side.
template <int K>
__global__ __launch_bounds__(256) void k_yuvp_unpack(const unsigned char* __restrict__ src, size_t pitch, unsigned w, unsigned cw,
                                                     unsigned rows, unsigned cpr, unsigned row_dwords, float* __restrict__ dy,
                                                     float* __restrict__ du, float* __restrict__ dv, float* __restrict__ da,
                                                     YuvPackedRule f, int io, int fvec)
{
    using S = PkShape<K>;
    const unsigned total = cpr * rows;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = i - r * cpr;
        const unsigned nd = min(4u, row_dwords - 4 * c);
        const unsigned char* p = src + (size_t)r * pitch + (size_t)16 * c;
        unsigned q[4] = {0, 0, 0, 0};
        if (nd == 4 && io == kIoVec) {
            const uint4 x = *reinterpret_cast<const uint4*>(p);
            q[0] = x.x; q[1] = x.y; q[2] = x.z; q[3] = x.w;
        } else {
            const int piece = io == kIoVec ? kIoDword : io;
#pragma unroll
            for (unsigned j = 0; j < 4; ++j)
                if (j < nd) q[j] = load_dword(p + 4 * j, piece);
        }
        unsigned y[8], u[4], v[4], a[4];
        decode<K>(q, f, y, u, v, a);
        float fy[8], fu[4], fv[4], fa[4];
#pragma unroll
        for (unsigned k = 0; k < S::NY; ++k) fy[k] = (float)y[k] * f.down;
#pragma unroll
        for (unsigned k = 0; k < S::NC; ++k) { fu[k] = (float)u[k]; fv[k] = (float)v[k]; }
#pragma unroll
        for (unsigned k = 0; k < S::NA; ++k) fa[k] = (float)a[k];
        const unsigned ny = valid_of(S::NY, c, w), nc = valid_of(S::NC, c, cw);
        store_floats<S::NY>(dy + (size_t)r * w + (size_t)S::NY * c, fy, ny, fvec);
        store_floats<S::NC>(du + (size_t)r * cw + (size_t)S::NC * c, fu, nc, fvec);
        store_floats<S::NC>(dv + (size_t)r * cw + (size_t)S::NC * c, fv, nc, fvec);
        if constexpr (S::NA > 0) store_floats<S::NA>(da + (size_t)r * w + (size_t)S::NA * c, fa, ny, fvec);
    }
}

// cpr: 16-byte chunks of a tight row (v210: its padding groups included).  Source row r of every plane goes to destination
// row row0 + r.
template <int K>
__global__ __launch_bounds__(256) void k_yuvp_pack(const float* __restrict__ sy, const float* __restrict__ su,
                                                   const float* __restrict__ sv, const float* __restrict__ sa, unsigned w,
                                                   unsigned cw, unsigned rows, unsigned cpr, unsigned row_dwords,
                                                   unsigned char* __restrict__ dst, size_t pitch, unsigned row0, YuvPackedRule f,
                                                   int io, int fvec)
{
    using S = PkShape<K>;
    const unsigned total = cpr * rows;
    const float maxv = (float)f.mask, amax = (float)f.amask;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const unsigned r = i / cpr, c = i - r * cpr;
        const unsigned nd = min(4u, row_dwords - 4 * c);
        const unsigned ny = valid_of(S::NY, c, w), nc = valid_of(S::NC, c, cw);
        float fy[8], fu[4], fv[4], fa[4];
        load_floats<S::NY>(sy + (size_t)r * w + (size_t)S::NY * c, fy, ny, fvec);
        load_floats<S::NC>(su + (size_t)r * cw + (size_t)S::NC * c, fu, nc, fvec);
        load_floats<S::NC>(sv + (size_t)r * cw + (size_t)S::NC * c, fv, nc, fvec);
        if constexpr (S::NA > 0) load_floats<S::NA>(sa + (size_t)r * w + (size_t)S::NA * c, fa, ny, fvec);
        unsigned y[8] = {0, 0, 0, 0, 0, 0, 0, 0}, u[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0}, a[4] = {0, 0, 0, 0};
#pragma unroll
        for (unsigned k = 0; k < S::NY; ++k) y[k] = k < ny ? to_word<false>(fy[k], f.up, maxv) : 0u;
#pragma unroll
        for (unsigned k = 0; k < S::NC; ++k) {
            u[k] = k < nc ? to_word<true>(fu[k], 1.f, maxv) : 0u;
            v[k] = k < nc ? to_word<true>(fv[k], 1.f, maxv) : 0u;
        }
#pragma unroll
        for (unsigned k = 0; k < S::NA; ++k) a[k] = k < ny ? to_word<true>(fa[k], 1.f, amax) : 0u;
        unsigned q[4];
        encode<K>(y, u, v, a, f, q);
        unsigned char* p = dst + (size_t)(row0 + r) * pitch + (size_t)16 * c;
        if (nd == 4 && io == kIoVec) {
            *reinterpret_cast<uint4*>(p) = make_uint4(q[0], q[1], q[2], q[3]);
        } else {
            const int piece = io == kIoVec ? kIoDword : io;
#pragma unroll
            for (unsigned j = 0; j < 4; ++j)
                if (j < nd) store_dword(p + 4 * j, q[j], piece);
        }
    }
}

// The row length that keeps every row start of every float plane aligned for the widest access its kind uses (float4 for 8
// and 4 samples, float2 for 6 and 2; 3 samples go one by one).
bool float_vec_ok(int kind, unsigned w)
{
    switch (kind) {
    case kPk422x8: return w % 8 == 0;    // Y: float4 at 8 per chunk; chroma w / 2 per row, float4
    case kPk422x16: return w % 4 == 0;   // Y: float4; chroma w / 2 per row, float2
    case kPk444x8:
    case kPk410: return w % 4 == 0;
    default: return w % 2 == 0;          // Y416: float2;  v210: float2 for Y
    }
}

}  // namespace

void launch_yuvp_unpack(const unsigned char* src, size_t pitch, unsigned w, unsigned rows, const YuvPackedRule& f, float* dy,
                        float* du, float* dv, float* da, hipStream_t s)
{
    const unsigned cw = yuv_packed_chroma_cols(f.kind, w);
    const size_t rb = yuv_packed_row_bytes(f.kind, w);
    const unsigned row_dwords = (unsigned)(rb / 4);
    const unsigned cpr = f.kind == kPkV210 ? (w + 5) / 6 : (unsigned)((rb + 15) / 16);   // v210: only the groups that carry a sample
    const int io = io_of(src, pitch);
    const int fvec = float_vec_ok(f.kind, w) && aligned_to(dy, 16) && aligned_to(du, 16) && aligned_to(dv, 16) && aligned_to(da, 16);
    const dim3 g = grid_for((size_t)cpr * rows, 4096), b(256);
#define SRCNN_YUVP_UNPACK(K) hipLaunchKernelGGL(k_yuvp_unpack<K>, g, b, 0, s, src, pitch, w, cw, rows, cpr, row_dwords, dy, du, dv, da, f, io, fvec)
    switch (f.kind) {
    case kPk422x8: SRCNN_YUVP_UNPACK(kPk422x8); break;
    case kPk422x16: SRCNN_YUVP_UNPACK(kPk422x16); break;
    case kPk444x8: SRCNN_YUVP_UNPACK(kPk444x8); break;
    case kPk410: SRCNN_YUVP_UNPACK(kPk410); break;
    case kPk444x16: SRCNN_YUVP_UNPACK(kPk444x16); break;
    default: SRCNN_YUVP_UNPACK(kPkV210); break;
    }
#undef SRCNN_YUVP_UNPACK
}

void launch_yuvp_pack(const float* sy, const float* su, const float* sv, const float* sa, unsigned w, unsigned rows,
                      const YuvPackedRule& f, unsigned char* dst, size_t pitch, unsigned row0, hipStream_t s, size_t span_bytes)
{
    const unsigned cw = yuv_packed_chroma_cols(f.kind, w);
    const size_t rb = span_bytes ? span_bytes : yuv_packed_row_bytes(f.kind, w);   // a rect: the chunks of its span and no more
    const unsigned row_dwords = (unsigned)(rb / 4);
    const unsigned cpr = (unsigned)((rb + 15) / 16);                 // every chunk of the tight row, v210's padding groups included
    const int io = io_of(dst, pitch);
    const int fvec = float_vec_ok(f.kind, w) && aligned_to(sy, 16) && aligned_to(su, 16) && aligned_to(sv, 16) && aligned_to(sa, 16);
    const dim3 g = grid_for((size_t)cpr * rows, 4096), b(256);
#define SRCNN_YUVP_PACK(K) hipLaunchKernelGGL(k_yuvp_pack<K>, g, b, 0, s, sy, su, sv, sa, w, cw, rows, cpr, row_dwords, dst, pitch, row0, f, io, fvec)
    switch (f.kind) {
    case kPk422x8: SRCNN_YUVP_PACK(kPk422x8); break;
    case kPk422x16: SRCNN_YUVP_PACK(kPk422x16); break;
    case kPk444x8: SRCNN_YUVP_PACK(kPk444x8); break;
    case kPk410: SRCNN_YUVP_PACK(kPk410); break;
    case kPk444x16: SRCNN_YUVP_PACK(kPk444x16); break;
    default: SRCNN_YUVP_PACK(kPkV210); break;
    }
#undef SRCNN_YUVP_PACK
}

}  // namespace srcnn
