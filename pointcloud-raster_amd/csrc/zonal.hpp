// zonal.hpp -- the arithmetic of the zonal tables (pcr_hip_zone_max, pcr_hip_zone_fold_stats, pcr_hip_zone_fold_hist,
// pcr_hip_zone_rows_stats, pcr_hip_zone_rows_percentiles, PipelineConfig::zonal), for the device (csrc/zonal.hip), the C-ABI's
// host twins and the host engine (host/src/zonal.cpp): all compile these lines, with contraction off, so a table folded in HBM
// and one folded by the host loop, and the rows made from either, agree bit for bit.  The contract is written in
// include/pcr_hip.h ("zonal tables") and DESIGN.md section 24.
//
// A zone is a set of cells that carry one label; the per-cell state is INTEGER planes (cell_stats.hpp: N, S1, S2; histogram.hpp:
// counts), so a zone's state is the integer sum of its cells' -- any order, any grouping, the same bits -- in 64-bit counters
// that wrap modulo 2^64.  The rows are the per-cell bands' arithmetic widened to a 64-bit count.
#pragma once

#include "cell_stats.hpp"
#include "histogram.hpp"

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PCR_ZN_HD __host__ __device__ __forceinline__
#else
#define PCR_ZN_HD inline
#endif

namespace pcrhip {
namespace zonal {

constexpr uint32_t kMaxZone = 1u << 24;         // PCR_HIP_ZONE_MAX: the greatest label a Float32 band holds exactly
constexpr int kMaxBins = hist::kMaxBins;
constexpr int kMaxPercentiles = hist::kMaxPercentiles;

// The zone of a cell: the label when it is a whole number in [1, 2^24], else 0 -- no zone.  NaN fails the first comparison,
// +-Inf, 0, -0.0 and negatives the range, 2.5 the floor, 2^24 + 1 is no Float32.
PCR_ZN_HD uint32_t zone_of(float v) {
    if (!(v >= 1.0f && v <= 16777216.0f)) return 0u;
    if (v != __builtin_floorf(v)) return 0u;
    return (uint32_t)v;
}

// D = n * S2 - S1^2 modulo 2^128, cs::numerator with a 64-bit n: one 64 x 64 -> 128 multiply for each term.
PCR_ZN_HD void numerator(uint64_t n, int64_t s1, uint64_t s2, uint64_t& hi, uint64_t& lo) {
    uint64_t ah, al, bh, bl;
    cs::mul64(n, s2, ah, al);
    const uint64_t a = s1 < 0 ? (uint64_t)0 - (uint64_t)s1 : (uint64_t)s1;
    cs::mul64(a, a, bh, bl);
    lo = al - bl;
    hi = ah - bh - (al < bl ? 1u : 0u);
}

// cs::bands_of with a 64-bit n: the same operations in the same order, every one rounded on its own.
PCR_ZN_HD void bands_of(uint64_t n, int64_t s1, uint64_t s2, double origin, double resolution, double res2, int ddof, float& mean,
                        float& variance, float& stddev) {
    mean = variance = stddev = cs::nodata();
    if (n == 0) return;
    const double mq = (double)s1 / (double)n;
    const double off = resolution * mq;
    mean = (float)(origin + off);
    if (n <= (uint64_t)ddof) return;
    uint64_t hi, lo;
    numerator(n, s1, s2, hi, lo);
    const double dh = (double)hi * 0x1p64;
    const double dd = dh + (double)lo;
    const double den = (double)n * (double)(n - (uint64_t)ddof);
    const double vq = dd / den;
    variance = (float)(res2 * vq);
    stddev = (float)(resolution * __builtin_sqrt(vq));
}

// hist::value_at with a 64-bit in_bin.
PCR_ZN_HD float value_at(double lo, double w, int b, int64_t k, uint64_t below, uint64_t in_bin) {
    const double pos = ((double)(k - (int64_t)below) - 0.5) / (double)in_bin;
    const double off = w * ((double)b + pos);
    return (float)(lo + off);
}

// The percentile q of one zone's row of `bins` counters whose sum is n: NaN where n == 0; else the rank of hist::rank_of, the
// smallest bin whose cumulative count reaches it, and value_at.  (n < 2^63, as rank_of's conversion asks.)
PCR_ZN_HD float percentile_of(const uint64_t* counts, int bins, uint64_t n, float q, double lo, double w) {
    if (n == 0) return hist::nodata();
    const int64_t k = hist::rank_of(q, n);
    uint64_t below = 0;
    for (int b = 0; b < bins; ++b) {
        const uint64_t c = counts[b];
        if (c != 0 && below + c >= (uint64_t)k) return value_at(lo, w, b, k, below, c);
        below += c;
    }
    return hist::nodata();                       // (not reached: the last bin's cumulative count is n >= k)
}

// ---- the host twins' loops: one thread, row-major, one add per cell ------------------------------------------------------------
inline uint32_t max_host(const float* zones, int w, int h, int64_t stride) {
    uint32_t m = 0;
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const uint32_t z = zone_of(zones[(int64_t)r * stride + c]);
            if (z > m) m = z;
        }
    return m;
}

// planes null: only `cells`; cells null: only the planes' tables.  A zone above Z is skipped.
inline void fold_stats_host(const float* zones, int w, int h, int64_t zone_stride, const uint32_t* pn, const long long* ps1,
                            const unsigned long long* ps2, int64_t plane_stride, uint32_t Z, unsigned long long* cells,
                            unsigned long long* zn, long long* zs1, unsigned long long* zs2) {
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const uint32_t z = zone_of(zones[(int64_t)r * zone_stride + c]);
            if (z == 0 || z > Z) continue;
            if (cells) cells[z - 1] += 1u;
            if (!pn) continue;
            const int64_t at = (int64_t)r * plane_stride + c;
            zn[z - 1] += (unsigned long long)pn[at];
            zs1[z - 1] = (long long)((unsigned long long)zs1[z - 1] + (unsigned long long)ps1[at]);
            zs2[z - 1] += ps2[at];
        }
}

inline void fold_hist_host(const float* zones, int w, int h, int64_t zone_stride, const uint32_t* counts, int bins,
                           int64_t count_stride, int64_t bin_stride, uint32_t Z, unsigned long long* zcounts) {
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const uint32_t z = zone_of(zones[(int64_t)r * zone_stride + c]);
            if (z == 0 || z > Z) continue;
            const uint32_t* cell = counts + (int64_t)r * count_stride + c;
            unsigned long long* row = zcounts + (std::size_t)(z - 1) * (std::size_t)bins;
            for (int b = 0; b < bins; ++b) row[b] += (unsigned long long)cell[(int64_t)b * bin_stride];
        }
}

}  // namespace zonal
}  // namespace pcrhip
