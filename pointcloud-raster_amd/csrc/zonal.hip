// zonal.hip -- zonal tables: the per-cell stats planes and histogram cubes folded by a label band into one row per zone
// (include/pcr_hip.h "zonal tables").  The arithmetic is csrc/zonal.hpp, which the host twins at the end
// of this file compile too.
//
// The folds are grouped reductions by atomics: one lane per cell, 64 consecutive cells per wave.  Neighbouring lanes with one
// label form a run; a segmented wave scan sums along each run and only the run's last lane adds to the zone's row, with 64-bit
// global atomic adds that return nothing.  The sums are integers, so any grouping of equal labels gives the same bits: runs may
// go on across a row end of a contiguous band, and combine = 0 (one set of atomics per cell) gives the same table.  The runs, the
// scan and the checks of Z, bins and the tables' spans are csrc/zone_fold.hpp, which the point folds (point_zonal.hip) share.
#include "zone_fold.hpp"

#include <algorithm>
#include <vector>

namespace pcrhip {
namespace {

namespace zn = zonal;
using namespace zfold;

constexpr int kBlock = 256;

struct Cells {                       // a band or plane of h rows of w elements, `stride` elements apart, as one lane per cell
    int w;
    int64_t n;                       // w * h
    __device__ __forceinline__ int64_t offset(int64_t i, int64_t stride) const {
        if (stride == w) return i;
        const int64_t r = i / w;
        return r * stride + (i - r * w);
    }
};

// ---- 1: the greatest zone of a band
__global__ __launch_bounds__(kBlock) void k_zone_max(const float* __restrict__ zones, Cells g, int64_t stride, uint32_t* out) {
    uint32_t m = 0;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + 3 * step < g.n; i += 4 * step) {                   // four loads in flight
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = zones[g.offset(i + k * step, stride)];
#pragma unroll
        for (int k = 0; k < 4; ++k) m = max(m, zn::zone_of(v[k]));
    }
    for (; i < g.n; i += step) m = max(m, zn::zone_of(zones[g.offset(i, stride)]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d));
    // One atomic per wave, and none where the word already holds as much: every wave strides over the whole band, so most
    // find their maximum there already (65536 atomics on the one word took fifty times a copy of the band).
    if ((threadIdx.x & 63) == 0 && m > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)__hip_atomic_fetch_max(out, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 2: cells, N, S1, S2 by zone
struct FoldStats {
    const float* zones;
    const uint32_t* pn;              // null: only `cells`
    const long long* ps1;
    const u64* ps2;
    int64_t zone_stride, plane_stride;
    Cells g;
    uint32_t Z;
    u64* cells;                      // null: only the planes' tables
    u64* zn;
    long long* zs1;
    u64* zs2;
};

template <bool COMBINE>
__global__ __launch_bounds__(kBlock) void k_zone_fold_stats(const FoldStats a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t z = i < a.g.n ? zn::zone_of(a.zones[a.g.offset(i, a.zone_stride)]) : 0u;
    if (z > a.Z) z = 0u;                                          // never an index into the table
    if (__ballot(z != 0u) == 0ull) return;                        // a wave with no zone loads nothing further
    u64 n = 0, s1 = 0, s2 = 0;
    if (z != 0u && a.pn) {
        const int64_t at = a.g.offset(i, a.plane_stride);
        n = a.pn[at];
        s1 = (u64)a.ps1[at];
        s2 = a.ps2[at];
    }
    u64 cells = 1;
    if (COMBINE) {
        const Run r = run_of(z);
        if (a.pn) {
            n = run_sum(r, n);
            s1 = run_sum(r, s1);
            s2 = run_sum(r, s2);
        }
        cells = (u64)(r.lane - r.start + 1);
        if (!r.tail) z = 0u;
    }
    if (z == 0u) return;
    if (a.cells) add_u64(a.cells + (z - 1), cells);
    if (a.pn) {
        add_u64(a.zn + (z - 1), n);
        add_u64(reinterpret_cast<u64*>(a.zs1) + (z - 1), s1);
        add_u64(a.zs2 + (z - 1), s2);
    }
}

// ---- 3: histogram counts by zone: the planes of the cube one after the other, each read coalesced
struct FoldHist {
    const float* zones;
    const uint32_t* counts;
    int64_t zone_stride, count_stride, bin_stride;
    Cells g;
    int bins;
    uint32_t Z;
    u64* zcounts;                    // [zone][bin]
};

template <bool COMBINE>
__global__ __launch_bounds__(kBlock) void k_zone_fold_hist(const FoldHist a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t z = i < a.g.n ? zn::zone_of(a.zones[a.g.offset(i, a.zone_stride)]) : 0u;
    if (z > a.Z) z = 0u;
    if (__ballot(z != 0u) == 0ull) return;
    const Run r = run_of(z);
    const uint32_t* cell = a.counts + (z != 0u ? a.g.offset(i, a.count_stride) : 0);
    u64* row = a.zcounts + (size_t)(z != 0u ? z - 1 : 0) * (size_t)a.bins;
    const bool adds = z != 0u && (!COMBINE || r.tail);
    for (int b0 = 0; b0 < a.bins; b0 += 4) {
        uint32_t c[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = z != 0u && b0 + k < a.bins ? cell[(int64_t)(b0 + k) * a.bin_stride] : 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (__ballot(c[k] != 0u) == 0ull) continue;          // (wave-uniform: a plane empty under this wave)
            const u64 v = COMBINE ? run_sum(r, (u64)c[k]) : (u64)c[k];
            if (adds && v != 0ull) add_u64(row + (b0 + k), v);
        }
    }
}

// ---- 4: the float columns, one lane per zone
struct RowsStats {
    const u64* zn;
    const long long* zs1;
    const u64* zs2;
    uint32_t Z;
    double origin, resolution, res2;
    int ddof;
    float* mean;
    float* var;
    float* sd;
};
__global__ __launch_bounds__(kBlock) void k_zone_rows_stats(const RowsStats a) {
    const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= a.Z) return;
    float m, v, s;
    zn::bands_of((uint64_t)a.zn[k], (int64_t)a.zs1[k], (uint64_t)a.zs2[k], a.origin, a.resolution, a.res2, a.ddof, m, v, s);
    if (a.mean) a.mean[k] = m;
    if (a.var) a.var[k] = v;
    if (a.sd) a.sd[k] = s;
}

struct RowsPct {
    const u64* zcounts;
    int bins;
    uint32_t Z;
    double lo, w;
    int n_q;
    float q[zn::kMaxPercentiles];
    u64* hist_n;
    float* out[zn::kMaxPercentiles];
};
// One WAVE per zone, so that a row of the table is read once and coalesced: lane L holds the bins [L * per, (L + 1) * per),
// per = ceil(bins / 64) <= 4.  A wave scan of the lanes' sums gives every lane the count below its first bin (integer sums:
// the cumulative counts of zonal::percentile_of's walk, whatever the grouping); per percentile every lane looks for the first of
// its bins that reaches the rank, and the lowest such lane -- the smallest such bin -- writes zonal::value_at.
constexpr int kZonesPerBlock = kBlock / 64;
__global__ __launch_bounds__(kBlock) void k_zone_rows_pct(const RowsPct a) {
    const uint32_t k = blockIdx.x * kZonesPerBlock + (threadIdx.x >> 6);
    if (k >= a.Z) return;                                         // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int per = (a.bins + 63) >> 6;
    const uint64_t* row = reinterpret_cast<const uint64_t*>(a.zcounts) + (size_t)k * (size_t)a.bins;
    uint64_t c[4] = {0, 0, 0, 0};
    uint64_t mine = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int b = lane * per + t;
        if (t < per && b < a.bins) c[t] = row[b];
        mine += c[t];
    }
    uint64_t upto = mine;                                         // the inclusive sum over lanes 0 .. L
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((long long)upto, d);
        if (lane >= d) upto += up;
    }
    const uint64_t n = (uint64_t)__shfl((long long)upto, 63);
    if (lane == 0 && a.hist_n) a.hist_n[k] = n;
    for (int j = 0; j < a.n_q; ++j) {
        if (n == 0) {
            if (lane == 0) a.out[j][k] = hist::nodata();
            continue;
        }
        const int64_t rank = hist::rank_of(a.q[j], n);
        uint64_t below = upto - mine;
        int hit = -1;
        uint64_t hit_below = 0, hit_count = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (hit < 0 && c[t] != 0 && below + c[t] >= (uint64_t)rank) {
                hit = t;
                hit_below = below;
                hit_count = c[t];
            }
            below += c[t];
        }
        const u64 found = __ballot(hit >= 0);
        if (found == 0ull) {                                      // (not reached: the last nonzero bin's cumulative count is n >= rank)
            if (lane == 0) a.out[j][k] = hist::nodata();
        } else if (lane == __ffsll((long long)found) - 1) {
            a.out[j][k] = zn::value_at(a.lo, a.w, lane * per + hit, rank, hit_below, hit_count);
        }
    }
}

// ---- the argument checks the entry points share
int check_cells(const std::string& fn, int width, int height) {
    PCR_REQUIRE((int64_t)width * height <= 2147483647LL, fn + ": more than 2^31 - 1 cells");
    return PCR_HIP_OK;
}

int check_max(const std::string& fn, const float* zones, int width, int height, int64_t stride, const uint32_t* out) {
    if (int rc = band::check_extent(fn, zones && out, width, height)) return rc;
    if (int rc = band::check_stride(fn, "zone", stride, width)) return rc;
    if (int rc = check_cells(fn, width, height)) return rc;
    PCR_REQUIRE(!overlap(span_of(zones, width, height, stride), span_of(out, 4)), fn + ": the result overlaps the zone band");
    return PCR_HIP_OK;
}

int check_fold_stats(const std::string& fn, const float* zones, int width, int height, int64_t zone_stride, const uint32_t* pn,
                     const long long* ps1, const unsigned long long* ps2, int64_t plane_stride, uint32_t Z,
                     const pcr_hip_zone_fold_params* params, const u64* cells, const u64* tn, const long long* ts1, const u64* ts2) {
    const bool planes = pn || ps1 || ps2 || tn || ts1 || ts2;
    const bool all = pn && ps1 && ps2 && tn && ts1 && ts2;
    if (int rc = band::check_extent(fn, zones && params && (planes ? all : cells != nullptr), width, height)) return rc;
    if (int rc = band::check_stride(fn, "zone", zone_stride, width)) return rc;
    if (planes)
        if (int rc = band::check_stride(fn, "plane", plane_stride, width)) return rc;
    if (int rc = check_Z(fn, Z)) return rc;
    if (int rc = check_cells(fn, width, height)) return rc;
    PCR_REQUIRE(params->combine == 0 || params->combine == 1, fn + ": combine must be 0 or 1");
    std::vector<Span> in{span_of(zones, width, height, zone_stride)}, tables;
    if (planes) {
        in.push_back(span_of(pn, width, height, plane_stride));
        in.push_back(span_of(ps1, width, height, plane_stride, 8));
        in.push_back(span_of(ps2, width, height, plane_stride, 8));
        tables.push_back(span_of(tn, (size_t)Z * 8));
        tables.push_back(span_of(ts1, (size_t)Z * 8));
        tables.push_back(span_of(ts2, (size_t)Z * 8));
    }
    if (cells) tables.push_back(span_of(cells, (size_t)Z * 8));
    return check_tables(fn, in, tables);
}

int check_fold_hist(const std::string& fn, const float* zones, int width, int height, int64_t zone_stride, const uint32_t* counts,
                    int bins, int64_t count_stride, int64_t bin_stride, uint32_t Z, const pcr_hip_zone_fold_params* params,
                    const u64* zcounts) {
    if (int rc = band::check_extent(fn, zones && counts && params && zcounts, width, height)) return rc;
    if (int rc = band::check_stride(fn, "zone", zone_stride, width)) return rc;
    if (int rc = band::check_stride(fn, "count", count_stride, width)) return rc;
    if (int rc = check_bins(fn, bins)) return rc;
    if (int rc = check_Z(fn, Z)) return rc;
    if (int rc = check_cells(fn, width, height)) return rc;
    PCR_REQUIRE(count_stride <= ((int64_t)1 << 40), fn + ": count_stride too large");
    const int64_t plane = (int64_t)(height - 1) * count_stride + width;
    PCR_REQUIRE(bin_stride >= plane && bin_stride <= ((int64_t)1 << 48), fn + ": bin_stride smaller than a plane of the cube");
    PCR_REQUIRE(params->combine == 0 || params->combine == 1, fn + ": combine must be 0 or 1");
    const Span table = span_of(zcounts, (size_t)Z * (size_t)bins * 8);
    const Span cube = span_of(counts, ((size_t)(bins - 1) * (size_t)bin_stride + (size_t)plane) * 4);
    PCR_REQUIRE(!overlap(table, span_of(zones, width, height, zone_stride)) && !overlap(table, cube), fn + ": the table overlaps an input");
    return PCR_HIP_OK;
}

int check_rows_stats(const std::string& fn, const u64* tn, const long long* ts1, const u64* ts2, uint32_t Z, double origin,
                     double resolution, int ddof, const float* mean, const float* var, const float* sd) {
    PCR_REQUIRE(tn && ts1 && ts2 && (mean || var || sd), fn + ": null argument");
    if (int rc = check_Z(fn, Z)) return rc;
    PCR_REQUIRE(std::isfinite(origin) && std::isfinite(resolution) && resolution > 0.0,
                fn + ": origin and resolution must be finite, the resolution positive");
    PCR_REQUIRE(ddof == 0 || ddof == 1, fn + ": ddof must be 0 or 1");
    const Span in[3] = {span_of(tn, (size_t)Z * 8), span_of(ts1, (size_t)Z * 8), span_of(ts2, (size_t)Z * 8)};
    for (const float* o : {mean, var, sd})
        for (const Span& s : in) PCR_REQUIRE(!o || !overlap(span_of(o, (size_t)Z * 4), s), fn + ": a column overlaps an input");
    return PCR_HIP_OK;
}

int check_rows_pct(const std::string& fn, const u64* zcounts, int bins, uint32_t Z, double lo, double w, int n_q, const float* q,
                   const u64* hist_n, float* const* outs) {
    PCR_REQUIRE(zcounts && (n_q == 0 || (q && outs)) && (n_q > 0 || hist_n), fn + ": null argument");
    if (int rc = check_bins(fn, bins)) return rc;
    if (int rc = check_Z(fn, Z)) return rc;
    PCR_REQUIRE(n_q >= 0 && n_q <= zn::kMaxPercentiles, fn + ": between 0 and 16 percentiles per call");
    PCR_REQUIRE(std::isfinite(lo) && std::isfinite(w) && w > 0.0, fn + ": lo and w must be finite, w positive");
    const Span in = span_of(zcounts, (size_t)Z * (size_t)bins * 8);
    PCR_REQUIRE(!hist_n || !overlap(span_of(hist_n, (size_t)Z * 8), in), fn + ": a column overlaps the table");
    for (int j = 0; j < n_q; ++j) {
        PCR_REQUIRE(q[j] >= 0.0f && q[j] <= 1.0f, fn + ": a percentile must lie in [0, 1]");
        PCR_REQUIRE(outs[j], fn + ": null output column");
        PCR_REQUIRE(!overlap(span_of(outs[j], (size_t)Z * 4), in), fn + ": a column overlaps the table");
    }
    return PCR_HIP_OK;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" {

int pcr_hip_zone_max(const float* d_zones, int width, int height, int64_t zone_stride, uint32_t* d_max, pcr_hip_stream s) {
    if (int rc = check_max("zone_max", d_zones, width, height, zone_stride, d_max)) return rc;
    hipStream_t st = static_cast<hipStream_t>(s);
    const Cells g{width, (int64_t)width * height};
    PCR_HIP_TRY(hipMemsetAsync(d_max, 0, sizeof(uint32_t), st));
    const unsigned blocks = (unsigned)std::min<int64_t>((g.n + 4 * kBlock - 1) / (4 * kBlock), 2048);
    hipLaunchKernelGGL(k_zone_max, dim3(std::max(blocks, 1u)), dim3(kBlock), 0, st, d_zones, g, zone_stride, d_max);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_zone_max_host(const float* h_zones, int width, int height, int64_t zone_stride, uint32_t* max) {
    if (int rc = check_max("zone_max_host", h_zones, width, height, zone_stride, max)) return rc;
    *max = zn::max_host(h_zones, width, height, zone_stride);
    return PCR_HIP_OK;
}

int pcr_hip_zone_fold_stats(const float* d_zones, int width, int height, int64_t zone_stride, const uint32_t* d_n, const long long* d_s1,
                            const unsigned long long* d_s2, int64_t plane_stride, uint32_t Z, const pcr_hip_zone_fold_params* params,
                            unsigned long long* d_cells, unsigned long long* d_zn, long long* d_zs1, unsigned long long* d_zs2,
                            pcr_hip_stream s) {
    if (int rc = check_fold_stats("zone_fold_stats", d_zones, width, height, zone_stride, d_n, d_s1, d_s2, plane_stride, Z, params,
                                  d_cells, d_zn, d_zs1, d_zs2))
        return rc;
    FoldStats a{};
    a.zones = d_zones;
    a.pn = d_n;
    a.ps1 = d_s1;
    a.ps2 = d_s2;
    a.zone_stride = zone_stride;
    a.plane_stride = d_n ? plane_stride : width;
    a.g = Cells{width, (int64_t)width * height};
    a.Z = Z;
    a.cells = d_cells;
    a.zn = d_zn;
    a.zs1 = d_zs1;
    a.zs2 = d_zs2;
    hipStream_t st = static_cast<hipStream_t>(s);
    if (params->combine) hipLaunchKernelGGL((k_zone_fold_stats<true>), dim3(blocks_of(a.g.n)), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_zone_fold_stats<false>), dim3(blocks_of(a.g.n)), dim3(kBlock), 0, st, a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_zone_fold_stats_host(const float* h_zones, int width, int height, int64_t zone_stride, const uint32_t* h_n,
                                 const long long* h_s1, const unsigned long long* h_s2, int64_t plane_stride, uint32_t Z,
                                 const pcr_hip_zone_fold_params* params, unsigned long long* h_cells, unsigned long long* h_zn,
                                 long long* h_zs1, unsigned long long* h_zs2) {
    if (int rc = check_fold_stats("zone_fold_stats_host", h_zones, width, height, zone_stride, h_n, h_s1, h_s2, plane_stride, Z, params,
                                  h_cells, h_zn, h_zs1, h_zs2))
        return rc;
    zn::fold_stats_host(h_zones, width, height, zone_stride, h_n, h_s1, h_s2, plane_stride, Z, h_cells, h_zn, h_zs1, h_zs2);
    return PCR_HIP_OK;
}

int pcr_hip_zone_fold_hist(const float* d_zones, int width, int height, int64_t zone_stride, const uint32_t* d_counts, int bins,
                           int64_t count_stride, int64_t bin_stride, uint32_t Z, const pcr_hip_zone_fold_params* params,
                           unsigned long long* d_zcounts, pcr_hip_stream s) {
    if (int rc = check_fold_hist("zone_fold_hist", d_zones, width, height, zone_stride, d_counts, bins, count_stride, bin_stride, Z,
                                 params, d_zcounts))
        return rc;
    FoldHist a{};
    a.zones = d_zones;
    a.counts = d_counts;
    a.zone_stride = zone_stride;
    a.count_stride = count_stride;
    a.bin_stride = bin_stride;
    a.g = Cells{width, (int64_t)width * height};
    a.bins = bins;
    a.Z = Z;
    a.zcounts = d_zcounts;
    hipStream_t st = static_cast<hipStream_t>(s);
    if (params->combine) hipLaunchKernelGGL((k_zone_fold_hist<true>), dim3(blocks_of(a.g.n)), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_zone_fold_hist<false>), dim3(blocks_of(a.g.n)), dim3(kBlock), 0, st, a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_zone_fold_hist_host(const float* h_zones, int width, int height, int64_t zone_stride, const uint32_t* h_counts, int bins,
                                int64_t count_stride, int64_t bin_stride, uint32_t Z, const pcr_hip_zone_fold_params* params,
                                unsigned long long* h_zcounts) {
    if (int rc = check_fold_hist("zone_fold_hist_host", h_zones, width, height, zone_stride, h_counts, bins, count_stride, bin_stride, Z,
                                 params, h_zcounts))
        return rc;
    zn::fold_hist_host(h_zones, width, height, zone_stride, h_counts, bins, count_stride, bin_stride, Z, h_zcounts);
    return PCR_HIP_OK;
}

int pcr_hip_zone_rows_stats(const unsigned long long* d_zn, const long long* d_zs1, const unsigned long long* d_zs2, uint32_t Z,
                            double origin, double resolution, int ddof, float* d_mean, float* d_var, float* d_std, pcr_hip_stream s) {
    if (int rc = check_rows_stats("zone_rows_stats", d_zn, d_zs1, d_zs2, Z, origin, resolution, ddof, d_mean, d_var, d_std)) return rc;
    const RowsStats a{d_zn, d_zs1, d_zs2, Z, origin, resolution, resolution * resolution, ddof, d_mean, d_var, d_std};
    hipLaunchKernelGGL(k_zone_rows_stats, dim3(blocks_of(Z)), dim3(kBlock), 0, static_cast<hipStream_t>(s), a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_zone_rows_stats_host(const unsigned long long* h_zn, const long long* h_zs1, const unsigned long long* h_zs2, uint32_t Z,
                                 double origin, double resolution, int ddof, float* h_mean, float* h_var, float* h_std) {
    if (int rc = check_rows_stats("zone_rows_stats_host", h_zn, h_zs1, h_zs2, Z, origin, resolution, ddof, h_mean, h_var, h_std)) return rc;
    const double res2 = resolution * resolution;
    for (uint32_t k = 0; k < Z; ++k) {
        float m, v, sd;
        zn::bands_of((uint64_t)h_zn[k], (int64_t)h_zs1[k], (uint64_t)h_zs2[k], origin, resolution, res2, ddof, m, v, sd);
        if (h_mean) h_mean[k] = m;
        if (h_var) h_var[k] = v;
        if (h_std) h_std[k] = sd;
    }
    return PCR_HIP_OK;
}

int pcr_hip_zone_rows_percentiles(const unsigned long long* d_zcounts, int bins, uint32_t Z, double lo, double w, int n_q, const float* q,
                                  unsigned long long* d_hist_n, float* const* d_outs, pcr_hip_stream s) {
    if (int rc = check_rows_pct("zone_rows_percentiles", d_zcounts, bins, Z, lo, w, n_q, q, d_hist_n, d_outs)) return rc;
    RowsPct a{};
    a.zcounts = d_zcounts;
    a.bins = bins;
    a.Z = Z;
    a.lo = lo;
    a.w = w;
    a.n_q = n_q;
    for (int j = 0; j < n_q; ++j) {
        a.q[j] = q[j];
        a.out[j] = d_outs[j];
    }
    a.hist_n = d_hist_n;
    hipLaunchKernelGGL(k_zone_rows_pct, dim3((Z + kZonesPerBlock - 1) / kZonesPerBlock), dim3(kBlock), 0, static_cast<hipStream_t>(s), a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_zone_rows_percentiles_host(const unsigned long long* h_zcounts, int bins, uint32_t Z, double lo, double w, int n_q,
                                       const float* q, unsigned long long* h_hist_n, float* const* h_outs) {
    if (int rc = check_rows_pct("zone_rows_percentiles_host", h_zcounts, bins, Z, lo, w, n_q, q, h_hist_n, h_outs)) return rc;
    for (uint32_t k = 0; k < Z; ++k) {
        const uint64_t* row = reinterpret_cast<const uint64_t*>(h_zcounts) + (size_t)k * (size_t)bins;
        uint64_t n = 0;
        for (int b = 0; b < bins; ++b) n += row[b];
        if (h_hist_n) h_hist_n[k] = n;
        for (int j = 0; j < n_q; ++j) h_outs[j][k] = zn::percentile_of(row, bins, n, q[j], lo, w);
    }
    return PCR_HIP_OK;
}

}  // extern "C"
