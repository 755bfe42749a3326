// histogram.hpp -- the per-cell value histogram's arithmetic (pcr_hip_scatter_histogram, pcr_hip_histogram_percentiles,
// PipelineConfig::histograms), for the device (csrc/histogram.hip), the C-ABI's host twin and the host engine
// (host/src/histogram.cpp): all compile these lines, with contraction off, so a cube counted in HBM and one counted by the
// host loop, and the bands walked out of either, agree bit for bit.  The contract is written in include/pcr_hip.h
// ("per-cell histograms") and DESIGN.md section 20.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCR_HIST_HD __host__ __device__ __forceinline__
#else
#define PCR_HIST_HD inline
#endif

namespace pcrhip {
namespace hist {

constexpr int kMaxBins = 256;                   // PCR_HIP_HISTOGRAM_MAX_BINS
constexpr int kMaxPercentiles = 16;             // PCR_HIP_HISTOGRAM_MAX_PERCENTILES
constexpr uint32_t kNoBin = 0xFFFFFFFFu;        // a NaN value: the point is not counted

// The bin of a value, binary64: t = (v - lo) * inv_w, one subtraction and one multiplication (nothing to contract); below
// the range, -Inf: bin 0; at or above it, +Inf: the last bin.  NaN: kNoBin.
PCR_HIST_HD uint32_t bin_of(float v, double lo, double inv_w, int bins) {
    if (v != v) return kNoBin;
    const double t = ((double)v - lo) * inv_w;
    if (t < 0.0) return 0u;
    if (t >= (double)bins) return (uint32_t)(bins - 1);
    return (uint32_t)(int)t;
}

PCR_HIST_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

// The rank the band for q reads among a cell's N >= 1 counted points: ceil(q * N) clamped to [1, N].
PCR_HIST_HD int64_t rank_of(float q, uint64_t n) {
    const double r = __builtin_ceil((double)q * (double)n);
    int64_t k = (int64_t)r;                      // (q in [0, 1] and N < 2^40: no overflow)
    if (k < 1) k = 1;
    if (k > (int64_t)n) k = (int64_t)n;
    return k;
}

// The band's value once the walk has found bin b: `below` points lie in the bins under it, `in_bin` >= 1 in it, the rank k is
// among them.  The k-th point is placed as if the bin's points were spread evenly: every operation rounded on its own.
PCR_HIST_HD float value_at(double lo, double w, int b, int64_t k, uint64_t below, uint32_t in_bin) {
    const double pos = ((double)(k - (int64_t)below) - 0.5) / (double)in_bin;
    const double off = w * ((double)b + pos);
    return (float)(lo + off);
}

}  // namespace hist
}  // namespace pcrhip
