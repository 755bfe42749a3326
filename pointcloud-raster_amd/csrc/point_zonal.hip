// point_zonal.hip -- point zonal tables: a value channel folded by a per-point label channel into one row per zone
// (include/pcr_hip.h "point zonal tables").  The arithmetic is csrc/point_zonal.hpp, which the host twins at
// the end of this file compile too.
//
// The tables are tiny and the cloud is huge: a few hundred to a few hundred thousand 64-bit rows against tens of millions of
// points of 9 bytes.  Persistent workgroups of 256 lanes stride over tiles of kTile = 1024 points, kInFlight tiles loaded before
// the first is used; label, mask and value are read once with non-temporal loads -- 16 bytes of label and of value and 4 mask
// bytes per lane where all three start on such a boundary (VEC: a lane owns four consecutive points), else element by element
// (a lane owns points t, t + 256, t + 512, t + 768 of the tile).  Per slot k of the four, the 64 lanes of a wave hold 64 points:
// neighbouring lanes with one zone (one zone and bin, for a histogram) form a run, a segmented wave scan sums along it, and the
// run's last lane adds the run's sums to the zone's row -- the run-combining of csrc/zone_fold.hpp, k_zone_fold_stats' too.  The
// sums are integers, so any grouping of equal labels gives the same bits, whether the lanes' points are neighbours in memory or not.
//   path 1  the row is in HBM: one set of 64-bit global atomic adds per run, no value returned.
//   path 2  the row is in a workgroup-private table in LDS, zeroed at the start: one set of LDS atomics per run; the workgroup
//           adds the table's NONZERO entries to HBM with global atomics at the end of its sweep.  An LDS row packs the count
//           with the sum -- n << 43 | sum of (q + 2^21), like k_cell_stats_tile's word A -- and counts points and bins in 32
//           bits: a workgroup therefore flushes and zeroes its table after every kEpochPoints = 2^20 points it has read, so that
//           n <= 2^20 < 2^21 and sum of (q + 2^21) <= 2^20 * 2^22 < 2^43.
// info: a lane keeps the greatest zone and the overflow count of its points; one wave reduction at the end of the sweep, the
// waves' results through LDS, and at most one agent-scope atomic max and one atomic add per workgroup.
#include "zone_fold.hpp"
#include "point_zonal.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace pcrhip {
namespace {

namespace pz = pzonal;
using namespace zfold;

constexpr int kBlock = PCR_HIP_POINT_FOLD_BLOCK;
constexpr int kPer = PCR_HIP_POINT_FOLD_POINTS_PER_LANE;
constexpr int kTile = kBlock * kPer;
constexpr int kInFlight = PCR_HIP_POINT_FOLD_TILES_IN_FLIGHT;
// (the element-wise variant keeps half as many: sixteen bounds and addresses of its own per lane did not fit the scalar registers)
template <bool VEC>
constexpr int in_flight() { return VEC ? kInFlight : kInFlight / 2; }
constexpr uint32_t kLdsBudget = PCR_HIP_POINT_FOLD_LDS_BYTES;
constexpr uint32_t kStatsRowBytes = PCR_HIP_POINT_FOLD_STATS_ROW_BYTES;    // word A, S2, points
constexpr uint32_t kEpochPoints = 1u << 20;
constexpr int kShift = 43;
constexpr int kBlocksPerCuGlobal = PCR_HIP_POINT_FOLD_BLOCKS_PER_CU_GLOBAL;
constexpr int kBlocksPerCuLds = PCR_HIP_POINT_FOLD_BLOCKS_PER_CU_LDS;
static_assert(kPer == 4, "the 16-byte accesses of the VEC variant cover four points");
static_assert(kInFlight % 2 == 0 && kEpochPoints % (kTile * kInFlight) == 0, "an epoch is whole trips");

__device__ __forceinline__ void lds_add_u64(u64* p, u64 v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_add_u32(uint32_t* p, uint32_t v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// ---- the points of one tile as a lane holds them
struct Slots {
    float label[kPer];
    float value[kPer];
    uint32_t keep;                   // bit k: slot k is a point of the cloud that the mask keeps
};

// Tile `tile` (any index: slots past the cloud's end are no points).  value null: not read.
template <bool VEC>
__device__ __forceinline__ void load_tile(const float* __restrict__ label, const uint8_t* __restrict__ mask, const float* __restrict__ value,
                                          uint64_t n, uint64_t tile, Slots& s) {
    const uint64_t base = tile * (uint64_t)kTile;
    const uint64_t first = VEC ? base + (uint64_t)(kPer * threadIdx.x) : base + (uint64_t)threadIdx.x;
    constexpr uint64_t step = VEC ? 1 : kBlock;
    if (VEC && first + kPer <= n) {
        const float4 l4 = stream_load(reinterpret_cast<const float4*>(label + first));
        s.label[0] = l4.x; s.label[1] = l4.y; s.label[2] = l4.z; s.label[3] = l4.w;
        if (value) {
            const float4 v4 = stream_load(reinterpret_cast<const float4*>(value + first));
            s.value[0] = v4.x; s.value[1] = v4.y; s.value[2] = v4.z; s.value[3] = v4.w;
        }
        s.keep = 0xFu;
        if (mask) {
            const uint32_t m = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(mask + first));
            s.keep = ((m & 0xFFu) ? 1u : 0u) | ((m & 0xFF00u) ? 2u : 0u) | ((m & 0xFF0000u) ? 4u : 0u) | ((m & 0xFF000000u) ? 8u : 0u);
        }
        return;
    }
    s.keep = 0u;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const uint64_t i = first + (uint64_t)k * step;
        const bool live = i < n;
        s.label[k] = live ? __builtin_nontemporal_load(label + i) : 0.0f;
        s.value[k] = live && value ? __builtin_nontemporal_load(value + i) : 0.0f;
        const bool kept = live && (!mask || __builtin_nontemporal_load(mask + i) != 0);
        s.keep |= kept ? (1u << k) : 0u;
    }
}

// ---- info: the lanes' greatest zone and overflow count, once per workgroup
__device__ __forceinline__ void info_leaves(uint32_t zmax, u64 over, u64* info) {
    __shared__ uint32_t sh_max[kBlock / 64];
    __shared__ u64 sh_over[kBlock / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        zmax = max(zmax, (uint32_t)__shfl_xor((int)zmax, d));
        over += (u64)__shfl_xor((long long)over, d);
    }
    if ((threadIdx.x & 63) == 0) {
        sh_max[threadIdx.x >> 6] = zmax;
        sh_over[threadIdx.x >> 6] = over;
    }
    __syncthreads();
    if (threadIdx.x != 0 || !info) return;
    u64 m = 0, o = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        m = max(m, (u64)sh_max[w]);
        o += sh_over[w];
    }
    if (m > __hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)__hip_atomic_fetch_max(info, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (o != 0) add_u64(info + 1, o);
}

extern __shared__ u64 lds_table[];

// ---- 1: points, n, s1, s2 by zone
struct FoldStats {
    const float* label;
    const uint8_t* mask;             // null: every point is kept
    const float* value;              // null: only `points`
    uint64_t n;
    double origin, inv_res;
    uint32_t Z;
    u64* points;                     // null: not counted
    u64* zn;
    long long* zs1;
    u64* zs2;
    u64* info;                       // null: not kept
};

// Path 2's table: word A of every zone, then S2, then the 32-bit point counts.
__device__ __forceinline__ void stats_table_zero(uint32_t Z) {
    for (uint32_t i = threadIdx.x; i < 2u * Z; i += kBlock) lds_table[i] = 0ull;
    uint32_t* p = reinterpret_cast<uint32_t*>(lds_table + 2u * Z);
    for (uint32_t i = threadIdx.x; i < Z; i += kBlock) p[i] = 0u;
}
__device__ __forceinline__ void stats_table_flush(const FoldStats& a) {
    const uint32_t Z = a.Z;
    uint32_t* p = reinterpret_cast<uint32_t*>(lds_table + 2u * Z);
    for (uint32_t k = threadIdx.x; k < Z; k += kBlock) {
        const uint32_t pts = p[k];
        if (pts == 0u) continue;                                 // (a zone without a point has no value either)
        p[k] = 0u;
        if (a.points) add_u64(a.points + k, (u64)pts);
        const u64 A = lds_table[k];
        if (A == 0ull) continue;
        const u64 S2 = lds_table[Z + k];
        lds_table[k] = 0ull;
        lds_table[Z + k] = 0ull;
        const u64 cnt = A >> kShift;
        const u64 su = A & ((1ull << kShift) - 1ull);            // the sum of q + 2^21
        add_u64(a.zn + k, cnt);
        add_u64(reinterpret_cast<u64*>(a.zs1) + k, su - cnt * (u64)cs::kQ);
        if (S2 != 0ull) add_u64(a.zs2 + k, S2);
    }
}

template <int PATH, bool VEC>
__global__ __launch_bounds__(kBlock) void k_point_fold_stats(const FoldStats a) {
    constexpr int F = in_flight<VEC>();
    const uint64_t tiles = (a.n + kTile - 1) / kTile;
    uint32_t zmax = 0, since = 0;
    u64 over = 0;
    if (PATH == 2) {
        stats_table_zero(a.Z);
        __syncthreads();
    }
    uint32_t* lds_points = reinterpret_cast<uint32_t*>(lds_table + 2u * a.Z);
    for (uint64_t t0 = blockIdx.x; t0 < tiles; t0 += (uint64_t)gridDim.x * F) {
        Slots s[F];
#pragma unroll
        for (int f = 0; f < F; ++f) load_tile<VEC>(a.label, a.mask, a.value, a.n, t0 + (uint64_t)f * gridDim.x, s[f]);
#pragma unroll
        for (int f = 0; f < F; ++f) {
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const pz::Where w = pz::where_of(s[f].label[k], (s[f].keep >> k) & 1u, a.Z);
                const uint32_t z = w.zone;
                over += w.over ? 1ull : 0ull;
                zmax = max(zmax, z);
                if (__ballot(z != 0u) == 0ull) continue;         // (wave-uniform)
                const Run r = run_of(z);
                const uint32_t pts = (uint32_t)(r.lane - r.start + 1);
                uint32_t cn = 0;
                int32_t c1 = 0;
                u64 c2 = 0;
                if (a.value) {
                    const int32_t q = z != 0u ? cs::step_of(s[f].value[k], a.origin, a.inv_res) : cs::kNoStep;
                    if (q != cs::kNoStep) {
                        cn = 1u;
                        c1 = q;
                        c2 = (u64)((long long)q * (long long)q);
                    }
                    cn = run_sum(r, cn);                         // (a wave's 64 steps: |sum| <= 2^27, in 32 bits)
                    c1 = run_sum(r, c1);
                    c2 = (u64)run_sum(r, (long long)c2);
                }
                if (!r.tail || z == 0u) continue;
                const uint32_t row = z - 1u;
                if (PATH == 2) {
                    lds_add_u32(lds_points + row, pts);
                    if (cn != 0u) {
                        lds_add_u64(lds_table + row, ((u64)cn << kShift) + (u64)((long long)c1 + (long long)cn * cs::kQ));
                        if (c2 != 0ull) lds_add_u64(lds_table + a.Z + row, c2);
                    }
                } else {
                    if (a.points) add_u64(a.points + row, (u64)pts);
                    if (cn != 0u) {
                        add_u64(a.zn + row, (u64)cn);
                        add_u64(reinterpret_cast<u64*>(a.zs1) + row, (u64)(long long)c1);
                        if (c2 != 0ull) add_u64(a.zs2 + row, c2);
                    }
                }
            }
        }
        if (PATH == 2) {
            since += (uint32_t)(kTile * F);
            if (since == kEpochPoints) {                         // the 32-bit and packed counters are full: flush, go on
                __syncthreads();
                stats_table_flush(a);
                __syncthreads();
                since = 0;
            }
        }
    }
    if (PATH == 2) {
        __syncthreads();
        stats_table_flush(a);
    }
    info_leaves(zmax, over, a.info);
}

// ---- 2: histogram counts by zone
struct FoldHist {
    const float* label;
    const uint8_t* mask;
    const float* value;
    uint64_t n;
    int bins;
    double lo, inv_w;
    uint32_t Z;
    u64* zcounts;                    // [zone][bin]
    u64* info;
};

__device__ __forceinline__ void hist_table_flush(const FoldHist& a) {
    uint32_t* c = reinterpret_cast<uint32_t*>(lds_table);
    const uint32_t words = a.Z * (uint32_t)a.bins;
    for (uint32_t i = threadIdx.x; i < words; i += kBlock) {
        const uint32_t v = c[i];
        if (v == 0u) continue;
        c[i] = 0u;
        add_u64(a.zcounts + i, (u64)v);
    }
}

template <int PATH, bool VEC>
__global__ __launch_bounds__(kBlock) void k_point_fold_hist(const FoldHist a) {
    constexpr int F = in_flight<VEC>();
    const uint64_t tiles = (a.n + kTile - 1) / kTile;
    uint32_t zmax = 0, since = 0;
    u64 over = 0;
    uint32_t* lds_counts = reinterpret_cast<uint32_t*>(lds_table);
    if (PATH == 2) {
        const uint32_t words = a.Z * (uint32_t)a.bins;
        for (uint32_t i = threadIdx.x; i < words; i += kBlock) lds_counts[i] = 0u;
        __syncthreads();
    }
    for (uint64_t t0 = blockIdx.x; t0 < tiles; t0 += (uint64_t)gridDim.x * F) {
        Slots s[F];
#pragma unroll
        for (int f = 0; f < F; ++f) load_tile<VEC>(a.label, a.mask, a.value, a.n, t0 + (uint64_t)f * gridDim.x, s[f]);
#pragma unroll
        for (int f = 0; f < F; ++f) {
#pragma unroll
            for (int k = 0; k < kPer; ++k) {
                const pz::Where w = pz::where_of(s[f].label[k], (s[f].keep >> k) & 1u, a.Z);
                over += w.over ? 1ull : 0ull;
                zmax = max(zmax, w.zone);
                uint32_t z = w.zone;
                const uint32_t b = z != 0u ? hist::bin_of(s[f].value[k], a.lo, a.inv_w, a.bins) : hist::kNoBin;
                if (b == hist::kNoBin) z = 0u;                   // a NaN value: in no run
                if (__ballot(z != 0u) == 0ull) continue;         // (wave-uniform)
                const Run r = run_of(z, b);
                if (!r.tail || z == 0u) continue;
                const uint32_t count = (uint32_t)(r.lane - r.start + 1);
                const size_t at = (size_t)(z - 1u) * (size_t)a.bins + b;
                if (PATH == 2) lds_add_u32(lds_counts + at, count);
                else add_u64(a.zcounts + at, (u64)count);
            }
        }
        if (PATH == 2) {
            since += (uint32_t)(kTile * F);
            if (since == kEpochPoints) {
                __syncthreads();
                hist_table_flush(a);
                __syncthreads();
                since = 0;
            }
        }
    }
    if (PATH == 2) {
        __syncthreads();
        hist_table_flush(a);
    }
    info_leaves(zmax, over, a.info);
}

// ---- the argument checks the entry points share (the spans, Z, bins and the tables: csrc/zone_fold.hpp)

// The greatest capacity path 2 takes: rows of kStatsRowBytes, or of 4 * bins bytes, in the LDS budget.
uint32_t lds_capacity(int bins) { return kLdsBudget / (bins > 0 ? 4u * (uint32_t)bins : kStatsRowBytes); }

// path 0 -> 2 where the table fits the budget, else 1.
int resolve_path(int path, uint32_t Z, int bins) { return path != 0 ? path : (Z <= lds_capacity(bins) ? 2 : 1); }

int check_common(const std::string& fn, uint32_t Z, int bins, const pcr_hip_point_fold_params* params) {
    if (int rc = check_Z(fn, Z)) return rc;
    PCR_REQUIRE(params->path >= 0 && params->path <= 2, fn + ": path must be 0 (auto), 1 (global atomics) or 2 (LDS table)");
    PCR_REQUIRE(params->path != 2 || Z <= lds_capacity(bins),
                fn + ": path 2 holds at most " + std::to_string(lds_capacity(bins)) + " zones of this row size in LDS");
    PCR_REQUIRE(params->blocks >= 0 && params->blocks <= 65536, fn + ": blocks must be between 0 (auto) and 65536");
    return PCR_HIP_OK;
}

int check_fold_stats(const std::string& fn, const float* label, const uint8_t* mask, const float* value, uint64_t n, double origin,
                     double inv_res, uint32_t Z, const pcr_hip_point_fold_params* params, const u64* points, const u64* zn,
                     const long long* zs1, const u64* zs2, const u64* info) {
    const bool any = value || zn || zs1 || zs2;
    const bool all = value && zn && zs1 && zs2;
    PCR_REQUIRE(label && params && (any ? all : points != nullptr), fn + ": null argument");
    if (int rc = check_common(fn, Z, 0, params)) return rc;
    PCR_REQUIRE(std::isfinite(origin) && std::isfinite(inv_res) && inv_res > 0.0, fn + ": origin and inv_res must be finite, inv_res positive");
    PCR_REQUIRE(n <= ((uint64_t)1 << 40), fn + ": more than 2^40 points in one call");
    std::vector<Span> in{span_of(label, n * 4)}, tables;
    if (mask) in.push_back(span_of(mask, n));
    if (value) in.push_back(span_of(value, n * 4));
    if (points) tables.push_back(span_of(points, (size_t)Z * 8));
    if (all) {
        tables.push_back(span_of(zn, (size_t)Z * 8));
        tables.push_back(span_of(zs1, (size_t)Z * 8));
        tables.push_back(span_of(zs2, (size_t)Z * 8));
    }
    if (info) tables.push_back(span_of(info, 16));
    return check_tables(fn, in, tables);
}

int check_fold_hist(const std::string& fn, const float* label, const uint8_t* mask, const float* value, uint64_t n, int bins, double lo,
                    double inv_w, uint32_t Z, const pcr_hip_point_fold_params* params, const u64* zcounts, const u64* info) {
    PCR_REQUIRE(label && value && params && zcounts, fn + ": null argument");
    if (int rc = check_bins(fn, bins)) return rc;
    if (int rc = check_common(fn, Z, bins, params)) return rc;
    PCR_REQUIRE(std::isfinite(lo) && std::isfinite(inv_w) && inv_w > 0.0, fn + ": lo and inv_w must be finite, inv_w positive");
    PCR_REQUIRE(n <= ((uint64_t)1 << 40), fn + ": more than 2^40 points in one call");
    std::vector<Span> in{span_of(label, n * 4), span_of(value, n * 4)}, tables{span_of(zcounts, (size_t)Z * (size_t)bins * 8)};
    if (mask) in.push_back(span_of(mask, n));
    if (info) tables.push_back(span_of(info, 16));
    return check_tables(fn, in, tables);
}

bool aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1u)) == 0; }

// The persistent workgroups of a launch: params->blocks, or blocks per CU by path, and never more than there are trips.
int blocks_of(const pcr_hip_point_fold_params* params, int path, uint64_t n, unsigned* blocks) {
    uint64_t want = (uint64_t)params->blocks;
    if (want == 0) {
        int dev = 0, cus = 0;
        PCR_HIP_TRY(hipGetDevice(&dev));
        PCR_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        want = (uint64_t)(path == 2 ? kBlocksPerCuLds : kBlocksPerCuGlobal) * (uint64_t)(cus > 0 ? cus : 256);
    }
    const uint64_t trips = (n + (uint64_t)kTile * kInFlight - 1) / ((uint64_t)kTile * kInFlight);
    *blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, trips));
    return PCR_HIP_OK;
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" {

int pcr_hip_point_fold_plan(uint32_t Z, int bins, uint64_t n, const pcr_hip_point_fold_params* params, int* path, int* blocks,
                            size_t* lds_bytes) {
    PCR_REQUIRE(params && path && blocks && lds_bytes, "point_fold_plan: null argument");
    PCR_REQUIRE(bins >= 0 && bins <= pz::kMaxBins, "point_fold_plan: bins must be between 0 (a stats fold) and 256");
    if (int rc = check_common("point_fold_plan", Z, bins, params)) return rc;
    *path = resolve_path(params->path, Z, bins);
    *lds_bytes = *path == 2 ? (size_t)Z * (bins > 0 ? 4u * (size_t)bins : (size_t)kStatsRowBytes) : 0;
    unsigned b = 0;
    if (int rc = blocks_of(params, *path, n, &b)) return rc;
    *blocks = (int)b;
    return PCR_HIP_OK;
}

int pcr_hip_point_fold_stats(const float* d_label, const uint8_t* d_mask, const float* d_value, uint64_t n, double origin, double inv_res,
                             uint32_t Z, const pcr_hip_point_fold_params* params, unsigned long long* d_points, unsigned long long* d_zn,
                             long long* d_zs1, unsigned long long* d_zs2, unsigned long long* d_info, pcr_hip_stream s) {
    if (int rc = check_fold_stats("point_fold_stats", d_label, d_mask, d_value, n, origin, inv_res, Z, params, d_points, d_zn, d_zs1,
                                  d_zs2, d_info))
        return rc;
    if (n == 0) return PCR_HIP_OK;
    const FoldStats a{d_label, d_mask, d_value, n, origin, inv_res, Z, d_points, d_zn, d_zs1, d_zs2, d_info};
    const int path = resolve_path(params->path, Z, 0);
    unsigned blocks = 0;
    if (int rc = blocks_of(params, path, n, &blocks)) return rc;
    const bool vec = aligned(d_label, 16) && (!d_value || aligned(d_value, 16)) && (!d_mask || aligned(d_mask, 4));
    const size_t lds = path == 2 ? (size_t)Z * kStatsRowBytes : 0;
    hipStream_t st = static_cast<hipStream_t>(s);
    if (path == 2) {
        if (vec) hipLaunchKernelGGL((k_point_fold_stats<2, true>), dim3(blocks), dim3(kBlock), lds, st, a);
        else hipLaunchKernelGGL((k_point_fold_stats<2, false>), dim3(blocks), dim3(kBlock), lds, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((k_point_fold_stats<1, true>), dim3(blocks), dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((k_point_fold_stats<1, false>), dim3(blocks), dim3(kBlock), 0, st, a);
    }
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_point_fold_stats_host(const float* h_label, const uint8_t* h_mask, const float* h_value, uint64_t n, double origin,
                                  double inv_res, uint32_t Z, const pcr_hip_point_fold_params* params, unsigned long long* h_points,
                                  unsigned long long* h_zn, long long* h_zs1, unsigned long long* h_zs2, unsigned long long* h_info) {
    if (int rc = check_fold_stats("point_fold_stats_host", h_label, h_mask, h_value, n, origin, inv_res, Z, params, h_points, h_zn, h_zs1,
                                  h_zs2, h_info))
        return rc;
    pz::fold_stats_host(h_label, h_mask, h_value, n, origin, inv_res, Z, h_points, h_zn, h_zs1, h_zs2, h_info);
    return PCR_HIP_OK;
}

int pcr_hip_point_fold_hist(const float* d_label, const uint8_t* d_mask, const float* d_value, uint64_t n, int bins, double lo, double inv_w,
                            uint32_t Z, const pcr_hip_point_fold_params* params, unsigned long long* d_zcounts, unsigned long long* d_info,
                            pcr_hip_stream s) {
    if (int rc = check_fold_hist("point_fold_hist", d_label, d_mask, d_value, n, bins, lo, inv_w, Z, params, d_zcounts, d_info)) return rc;
    if (n == 0) return PCR_HIP_OK;
    const FoldHist a{d_label, d_mask, d_value, n, bins, lo, inv_w, Z, d_zcounts, d_info};
    const int path = resolve_path(params->path, Z, bins);
    unsigned blocks = 0;
    if (int rc = blocks_of(params, path, n, &blocks)) return rc;
    const bool vec = aligned(d_label, 16) && aligned(d_value, 16) && (!d_mask || aligned(d_mask, 4));
    const size_t lds = path == 2 ? (size_t)Z * (size_t)bins * 4 : 0;
    hipStream_t st = static_cast<hipStream_t>(s);
    if (path == 2) {
        if (vec) hipLaunchKernelGGL((k_point_fold_hist<2, true>), dim3(blocks), dim3(kBlock), lds, st, a);
        else hipLaunchKernelGGL((k_point_fold_hist<2, false>), dim3(blocks), dim3(kBlock), lds, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((k_point_fold_hist<1, true>), dim3(blocks), dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((k_point_fold_hist<1, false>), dim3(blocks), dim3(kBlock), 0, st, a);
    }
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_point_fold_hist_host(const float* h_label, const uint8_t* h_mask, const float* h_value, uint64_t n, int bins, double lo,
                                 double inv_w, uint32_t Z, const pcr_hip_point_fold_params* params, unsigned long long* h_zcounts,
                                 unsigned long long* h_info) {
    if (int rc = check_fold_hist("point_fold_hist_host", h_label, h_mask, h_value, n, bins, lo, inv_w, Z, params, h_zcounts, h_info)) return rc;
    pz::fold_hist_host(h_label, h_mask, h_value, n, bins, lo, inv_w, Z, h_zcounts, h_info);
    return PCR_HIP_OK;
}

}  // extern "C"
