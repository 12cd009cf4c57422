// srcnn_y_path_geom.hpp -- the geometry of the Y path (resample, layers 1+2, layer 3) that every entry point shares: the halo
// of an output range, the source span of a range of a resampled axis, the size limits, and the band a pass may take under the
// workspace budget.  Plain arithmetic -- no HIP, no table builder -- so the stand-alone sanitizer programs under tests/host/
// include it (tests/host/y_path_geom_sanitize.cpp checks it against restatements).  Internal.
#pragma once
#include <algorithm>
#include <cstddef>

namespace srcnn {

constexpr unsigned kConv3Halo = 2;      // layer 3 is 5x5
constexpr unsigned kConv1Halo = 4;      // layer 1 is 9x9 (layer 2 is 1x1: none)
constexpr unsigned kLayer2Planes = 32;  // C2N of srcnn_kernels.h, which this header cannot include
constexpr unsigned kMaxGridRows = 65535u * 16u;      // rows one launch of the layer kernels covers: grid.y x one 16-row tile

// What the Y path computes for output indices [a,b) of an axis of `len`: layer-2 activations [ca,cb) = the range +-2 (layer 3
// clamps the ACTIVATIONS to the edge at the true border), and upscaled Y [ua,ub) = that +-4 for layer 1, cut at the borders.
struct HaloSpan {
    unsigned ca, cb, ua, ub;
    unsigned width() const { return ub - ua; }      // Ww of a column range: the width of the window the layers run over
};
inline HaloSpan y_path_halo(unsigned len, unsigned a, unsigned b)
{
    HaloSpan s;
    s.ca = a >= kConv3Halo ? a - kConv3Halo : 0;
    s.cb = std::min(len, b + kConv3Halo);
    s.ua = s.ca >= kConv1Halo ? s.ca - kConv1Halo : 0;
    s.ub = std::min(len, s.cb + kConv1Halo);
    return s;
}

// [lo,hi) of a source axis of src_len that destination indices [a,b) read: the taps of the range, read off the axis's
// contribution table (first[], taps[]), so exact for every filter and ratio
inline void taps_span(const int* first, const int* taps, unsigned src_len, unsigned a, unsigned b, unsigned& lo, unsigned& hi)
{
    int l = 0x7fffffff, e = 0;
    for (unsigned u = a; u < b; ++u) { l = std::min(l, first[u]); e = std::max(e, first[u] + taps[u]); }
    lo = (unsigned)l;
    hi = std::min((unsigned)e, src_len);
}

// The size limits of the Y path for `rows` output rows of a dw x dh result from a plane of h rows and src_samples = w * h
// samples (0: the caller's plane check has bounded them already)
inline bool y_path_fits(unsigned long long src_samples, unsigned h, unsigned dw, unsigned dh, unsigned rows)
{
    return h <= (1u << 20) && dh <= (1u << 20) && dw <= 0x7fffffu && rows <= kMaxGridRows && src_samples <= 0x7fffffffULL;
}

// Rows one pass of the Y path produces of `rows` rows over a window W floats wide: all of them when the fused tier runs (it has
// no layer-2 planes) or the 32 planes with their 4 halo rows fit `budget` bytes, else the band that fits -- at least 16 rows,
// one tile row of the layer kernels (a smaller budget is exceeded rather than refused; srcnn_amd.h says so).
inline unsigned y_path_band_rows(size_t budget, bool fused, unsigned W, unsigned rows)
{
    const size_t row_bytes = (size_t)kLayer2Planes * W * sizeof(float);
    if (fused || row_bytes * ((size_t)rows + 4) <= budget) return rows;
    const size_t fit = budget / row_bytes;
    return (unsigned)std::min<size_t>(rows, std::min<size_t>(std::max<size_t>(16, fit > 4 ? fit - 4 : 1), 1u << 20));
}

}  // namespace srcnn
