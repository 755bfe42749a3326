// fill_nodata.hpp -- the per-cell arithmetic of fill_nodata, for the device (csrc/fill_nodata.hip) and the host
// (host/src/fill_nodata.cpp): both compile these lines, so a band filled in HBM and one filled by the host loop agree bit for bit.
//
// fill(src, R), 1 <= R <= kMaxRadius, out of place.  A cell that is not NaN is copied bit for bit.  For a NaN cell at (r, c)
// the window offsets are visited in row-major order, dr = -R..R and inside it dc = -R..R; an offset is skipped when
// d2 = dr*dr + dc*dc is 0 or greater than R*R, when (r+dr, c+dc) is outside the image, or when the source cell there is NaN.
// Every other offset contributes with w = 1.0f / (float)d2 (a correctly rounded binary32 division) to two binary64 sums that
// start at +0.0:  s += (double)w * (double)v;  t += (double)w.  The product of two binary32 numbers is exact in binary64, so
// fma and mul + add give the same bits: only the ORDER of the additions is part of the contract.
//   t == 0     nothing valid in range: the source NaN, bit for bit (payload included)
//   otherwise  (float)(s / t): a true binary64 division, then round to nearest even; a NaN result (Inf + -Inf among the
//              neighbours) is the one pattern 0x7FC00000 (as overview.hpp: machines disagree on that NaN's sign bit).
// +-Inf and denormals are ordinary values.  Filling never chains: every read is of src, a hole wider than 2R keeps a NaN core.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCR_FILL_HD __host__ __device__ __forceinline__
#else
#define PCR_FILL_HD inline
#endif

namespace pcrhip {
namespace fill {

constexpr int kMaxRadius = 32;

PCR_FILL_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

// the weight of an offset with squared distance d2 (1 <= d2 <= kMaxRadius^2)
PCR_FILL_HD float weight(int d2) { return 1.0f / (float)d2; }

// the greatest |dc| inside the disc on the window row |dr| = a: dc*dc + a*a <= R*R
PCR_FILL_HD int half_width(int R, int a) {
    int k = 0;
    while (k < R && (k + 1) * (k + 1) + a * a <= R * R) ++k;
    return k;
}

// one valid neighbour (v is not NaN) of weight w
PCR_FILL_HD void accumulate(double& s, double& t, float w, float v) {
    s += (double)w * (double)v;
    t += (double)w;
}

// the filled value of a NaN cell `src` from its sums
PCR_FILL_HD float finish(double s, double t, float src) {
    if (t == 0.0) return src;
    const float r = (float)(s / t);
    return r != r ? nodata() : r;
}

}  // namespace fill
}  // namespace pcrhip
