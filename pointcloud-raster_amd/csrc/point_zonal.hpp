// point_zonal.hpp -- the arithmetic of the POINT zonal tables (pcr_hip_point_fold_stats, pcr_hip_point_fold_hist,
// PipelineConfig::point_zonal, pcr.point_zonal), for the device (csrc/point_zonal.hip), the C-ABI's host twins and the host
// engine (host/src/point_zonal.cpp): all compile these lines, with contraction off, so a table folded in HBM and one folded by
// the host loop agree bit for bit.  The contract is written in include/pcr_hip.h ("point zonal tables") and DESIGN.md section 27.
//
// A zone is a set of POINTS that carry one label in a per-point Float32 channel; a point's contribution is integers
// (cell_stats.hpp: the step q; histogram.hpp: the bin), so a zone's state is an integer sum over its points -- any order, any
// chunking, any path, the same bits -- in 64-bit counters that wrap modulo 2^64.  The grid plays no part: neither x nor y is
// read.  The rows are zonal.hpp's (bands_of, percentile_of), unchanged.
#pragma once

#include "zonal.hpp"

#include <cstddef>
#include <cstdint>

namespace pcrhip {
namespace pzonal {

constexpr uint32_t kMaxZone = zonal::kMaxZone;
constexpr int kMaxBins = hist::kMaxBins;

// What a point is for a table of capacity Z.  kept: its mask byte is nonzero (or there is no mask).
//   zone 1..Z   the point's row is zone - 1
//   0           no zone: masked out, or a label that is none (NaN, +-Inf, 0, -0.0, negatives, fractions)
//   over        a mask-kept point whose zone is above Z: never an index, counted in info[1]
struct Where {
    uint32_t zone;
    bool over;
};
PCR_ZN_HD Where where_of(float label, bool kept, uint32_t Z) {
    Where w{0u, false};
    if (!kept) return w;
    const uint32_t z = zonal::zone_of(label);
    if (z > Z) w.over = true;
    else w.zone = z;
    return w;
}

// ---- the host twins' loops: one thread, one add per point --------------------------------------------------------------------
// info (two words, or null): info[0] = max(info[0], the greatest zone <= Z a mask-kept point carried), info[1] += the number of
// mask-kept points with a zone above Z.  points null: not counted; value null (with zn, zs1, zs2): only `points`.
inline void fold_stats_host(const float* label, const uint8_t* mask, const float* value, uint64_t n, double origin, double inv_res,
                            uint32_t Z, unsigned long long* points, unsigned long long* zn, long long* zs1, unsigned long long* zs2,
                            unsigned long long* info) {
    for (uint64_t i = 0; i < n; ++i) {
        const Where w = where_of(label[i], !mask || mask[i] != 0, Z);
        if (w.over && info) info[1] += 1u;
        if (w.zone == 0u) continue;
        const size_t k = (size_t)(w.zone - 1u);
        if (info && w.zone > info[0]) info[0] = w.zone;
        if (points) points[k] += 1u;
        if (!value) continue;
        const int32_t q = cs::step_of(value[i], origin, inv_res);
        if (q == cs::kNoStep) continue;
        zn[k] += 1u;
        zs1[k] = (long long)((unsigned long long)zs1[k] + (unsigned long long)(long long)q);
        zs2[k] += (unsigned long long)((long long)q * (long long)q);
    }
}

inline void fold_hist_host(const float* label, const uint8_t* mask, const float* value, uint64_t n, int bins, double lo, double inv_w,
                           uint32_t Z, unsigned long long* zcounts, unsigned long long* info) {
    for (uint64_t i = 0; i < n; ++i) {
        const Where w = where_of(label[i], !mask || mask[i] != 0, Z);
        if (w.over && info) info[1] += 1u;
        if (w.zone == 0u) continue;
        if (info && w.zone > info[0]) info[0] = w.zone;
        const uint32_t b = hist::bin_of(value[i], lo, inv_w, bins);
        if (b == hist::kNoBin) continue;
        zcounts[(size_t)(w.zone - 1u) * (size_t)bins + b] += 1u;
    }
}

}  // namespace pzonal
}  // namespace pcrhip
