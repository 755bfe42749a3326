// overview.hpp -- the per-cell arithmetic of a GeoTIFF overview level, for the device (csrc/overview.hip) and the host
// (host/src/overviews.cpp): both compile these lines, so a pyramid built in HBM and one built by the host loop agree bit for bit.
//
// Level k is made from level k-1 (level 0 is the band): cell (r, c) looks at a = (2r, 2c), b = (2r, 2c+1), c = (2r+1, 2c),
// d = (2r+1, 2c+1) of its source.  A cell outside the source, or a NaN cell, is invalid.
//   average   every invalid cell contributes +0.0f; s = ((a + b) + c) + d in binary32, in this order; n = number of valid
//             cells; the result is s / (float)n, a true (correctly rounded) division -- no reciprocal, no contraction.  n == 0
//             gives NaN.  +-Inf are values: Inf + -Inf is IEEE's invalid operation, whose NaN differs between machines in its
//             sign bit (x86 sets it, gfx9 does not), so EVERY NaN this function makes is the one pattern 0x7FC00000.
//   nearest   cell a, copied bit for bit (a NaN keeps its payload).
// The caller passes NaN for a cell outside the source.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCR_OVERVIEW_HD __host__ __device__ __forceinline__
#else
#define PCR_OVERVIEW_HD inline
#endif

namespace pcrhip {
namespace overview {

enum : int { kAverage = 0, kNearest = 1 };

// levels halve 64 -> 1 inside one source tile: a 64-aligned tile never splits a 2x2 window of levels 1..6
constexpr int kTile = 64;
constexpr int kLevelsPerPass = 6;

PCR_OVERVIEW_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

PCR_OVERVIEW_HD float average4(float a, float b, float c, float d) {
    const bool va = a == a, vb = b == b, vc = c == c, vd = d == d;
    const float s = (((va ? a : 0.0f) + (vb ? b : 0.0f)) + (vc ? c : 0.0f)) + (vd ? d : 0.0f);
    const int n = (int)va + (int)vb + (int)vc + (int)vd;
    if (n == 0 || s != s) return nodata();
    return s / (float)n;
}

PCR_OVERVIEW_HD float down4(int mode, float a, float b, float c, float d) {
    return mode == kNearest ? a : average4(a, b, c, d);
}

// size of level k of an n-cell axis: ceil applied k times == ceil(n / 2^k)
PCR_OVERVIEW_HD int level_extent(int n, int k) { return k >= 31 ? 1 : (int)(((int64_t)n + ((int64_t)1 << k) - 1) >> k); }

// number of halvings until the image is 1x1 (0 for a 1x1 image): the most levels an image has
PCR_OVERVIEW_HD int max_levels(int w, int h) {
    int k = 0;
    while (level_extent(w, k) > 1 || level_extent(h, k) > 1) ++k;
    return k;
}

}  // namespace overview
}  // namespace pcrhip
