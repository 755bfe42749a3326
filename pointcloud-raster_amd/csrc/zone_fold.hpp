// zone_fold.hpp -- what the two fold files share (zonal.hip: one lane per cell; point_zonal.hip: one slot per point): the runs of
// a wave and the segmented scan along them, the 64-bit atomic add that returns nothing, and the checks of Z, of bins and of the
// tables against their inputs that the entry points of both start with.  The spans are band_pass.hpp's.
#pragma once

#include "band_pass.hpp"
#include "zonal.hpp"

#include <vector>

namespace pcrhip {
namespace zfold {

using band::overlap;
using band::Span;
using band::span_of;

inline int check_Z(const std::string& fn, uint32_t Z) {
    PCR_REQUIRE(Z >= 1u && Z <= zonal::kMaxZone, fn + ": Z must be between 1 and 2^24");
    return PCR_HIP_OK;
}
inline int check_bins(const std::string& fn, int bins) {
    PCR_REQUIRE(bins >= 1 && bins <= zonal::kMaxBins, fn + ": bins must be between 1 and 256");
    return PCR_HIP_OK;
}
// No table overlaps an input or another table.  (An empty span overlaps nothing: a fold of no points may name one buffer twice.)
inline int check_tables(const std::string& fn, const std::vector<Span>& in, const std::vector<Span>& tables) {
    for (size_t t = 0; t < tables.size(); ++t) {
        for (const Span& s : in) PCR_REQUIRE(!overlap(tables[t], s), fn + ": a table overlaps an input");
        for (size_t u = 0; u < t; ++u) PCR_REQUIRE(!overlap(tables[t], tables[u]), fn + ": two tables overlap");
    }
    return PCR_HIP_OK;
}

#if defined(__HIPCC__)
using u64 = unsigned long long;

__device__ __forceinline__ void add_u64(u64* p, u64 v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The runs of a wave: lane L heads a run when L == 0 or its key -- a zone, or a zone and a bin -- differs from lane L - 1's.
// `start` is the head of L's run, `tail` says L is its last lane.  (Lanes with nothing to add carry zone 0, like every cell or
// point with no zone.)
struct Run {
    int lane, start;
    bool tail;
};
__device__ __forceinline__ Run run_from(bool head) {
    Run r;
    r.lane = threadIdx.x & 63;
    const u64 heads = __ballot(r.lane == 0 || head);
    r.start = 63 - __clzll((long long)(heads & (~0ull >> (63 - r.lane))));
    r.tail = r.lane == 63 || ((heads >> (r.lane + 1)) & 1ull);
    return r;
}
__device__ __forceinline__ Run run_of(uint32_t z) { return run_from((uint32_t)__shfl_up((int)z, 1) != z); }
__device__ __forceinline__ Run run_of(uint32_t z, uint32_t b) {
    const uint32_t pz = (uint32_t)__shfl_up((int)z, 1), pb = (uint32_t)__shfl_up((int)b, 1);
    return run_from(pz != z || pb != b);
}
// The inclusive sum of v along the run: six steps; a lane takes lane - d's partial sum while that lane is inside its run.
template <class T>
__device__ __forceinline__ T run_sum(const Run& r, T v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = (T)__shfl_up(v, d);
        if (r.lane - d >= r.start) v += up;
    }
    return v;
}
#endif  // __HIPCC__

}  // namespace zfold
}  // namespace pcrhip
