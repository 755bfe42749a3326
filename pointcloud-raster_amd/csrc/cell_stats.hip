// cell_stats.hip -- per-cell spread (the contract: cell_stats.hpp, include/pcr_hip.h "per-cell stats"): the two scatter paths
// behind pcr_hip_scatter_cell_stats, and pcr_hip_cell_stats_bands with its host twin.
//
// State: three planes in the state window's layout, all zero at create: N (uint32, += 1), S1 (int64, += q) and S2 (uint64,
// += q * q), q the step of the value (cs::step_of, |q| <= Q = 2^21).  The fold is integer addition, so every path, order and
// chunking gives the same bits.
//   direct   k_stat_direct: route, step, three no-return global atomic adds (one 32-bit, two 64-bit).
//   binned   the Point front end unchanged (through sweep_tiles), as the histogram uses it: a streaming pre-pass (k_stat_steps)
//            turns every value into one 32-bit word, its step (kNoStep for a NaN), and that word rides through the scatter pass
//            in the VALUE slot of ordinary 8-byte records {local cell, step}.  The tile pass (k_tile_stats) folds an item's
//            records into an LDS tile of 128 x 72 cells with TWO 64-bit LDS atomic adds per record, on u = q + Q in [0, 2^22]:
//              word A   count << 47 | sum of u     an item is at most 2^16 records: sum of u <= 2^38 < 2^47, count <= 2^16
//              word B   sum of u^2                 <= 2^16 * 2^44 = 2^60
//            so neither field can carry into another: correct by construction.  The two words are kept PLANE-MAJOR (A[cells]
//            then B[cells]): the records of a tile hit random cells, and a 64-bit access takes the bank pair of its address,
//            so the 64 lanes of either atomic spread over all the banks as cell % 32 does; interleaved per cell (16 bytes)
//            each of the two instructions would use only every other bank pair.  Plane-major rows are also contiguous runs
//            the merge reads 16 bytes wide.  16 bytes a cell: 144 KB of LDS.
//            Merge: n, sum u, sum u^2 decoded; sum q = sum u - n Q and sum q^2 = sum u^2 - 2 Q sum u + n Q^2 in wrapping
//            64-bit arithmetic (exact: the true values fit).  An exclusively owned item adds them into the three planes with
//            plain wide read-modify-writes and skips cells no record hit; an item the scan split uses global atomics.
#include "engine.hpp"
#include "cell_stats.hpp"

#include <algorithm>
#include <cmath>

using namespace pcrhip;

namespace {

constexpr int kBlock = 256;
constexpr int kThreads = 1024;                    // full-CU workgroups, as the Point tile pass
constexpr int kStatTileW = 128;                   // a row of one word plane of a tile: a contiguous 1024-byte run
constexpr int kStatCellBytes = 16;                // words A and B
// A bin with more records than this is split into several work items, which then merge with atomics.  The LDS words' field
// widths are sized for it: do not raise it without them.
constexpr unsigned kStatItemRecords = 1u << 16;
constexpr int kCountShift = 47;
using u64 = unsigned long long;
constexpr u64 kSumMask = ((u64)1 << kCountShift) - 1;
static_assert((u64)kStatItemRecords * (2 * (u64)cs::kQ) < ((u64)1 << kCountShift), "an item's sum of u must stay below the count");
static_assert((((u64)kStatItemRecords << kCountShift) >> kCountShift) == kStatItemRecords, "an item's count must fit above the sum");
static_assert((u64)kStatItemRecords * (2 * (u64)cs::kQ) * (2 * (u64)cs::kQ) / (2 * (u64)cs::kQ) / (2 * (u64)cs::kQ) == kStatItemRecords,
              "an item's sum of u^2 must fit 64 bits");

// ---- direct path -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_stat_direct(GridDev g, uint32_t* __restrict__ pn, u64* __restrict__ ps1, u64* __restrict__ ps2, double origin, double inv_res,
              const double* __restrict__ x, const double* __restrict__ y, const float* __restrict__ v, uint64_t n,
              uint32_t* __restrict__ touched, unsigned long long* __restrict__ counters) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t n_round = ((n + 63) / 64) * 64;                // every lane of a wave runs the same trips (ballot inside)
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_round; i += stride) {
        bool valid = false;
        int col = 0, row = 0;
        if (i < n) {
            valid = point_kept(g, i) && world_to_cell(g, x[i], y[i], col, row);
            valid = valid && row >= g.own_r0 && row < g.own_r1;
        }
        if (valid) {
            const int32_t q = cs::step_of(v[i], origin, inv_res);
            if (q != cs::kNoStep) {                               // (the results are unused: atomics without return)
                const int64_t cell = (int64_t)(row - g.st_r0) * g.W + col;
                const int64_t q64 = q;
                atomicAdd(pn + cell, 1u);
                atomicAdd(ps1 + cell, (u64)q64);                  // (two's complement: the unsigned add is the signed one)
                atomicAdd(ps2 + cell, (u64)(q64 * q64));
            }
            touch_tile(g, touched, row, col);
        }
        const unsigned long long m = __ballot(valid);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(counters, (unsigned long long)__popcll(m));
    }
}

// ---- binned path -----------------------------------------------------------------------------------------------------------
// words[i] = step of v[i], kNoStep for a NaN: 4 B read and 4 B written per point, streaming.  VEC: four points per lane.
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
k_stat_steps(const float* __restrict__ v, uint32_t* __restrict__ words, uint64_t n, double origin, double inv_res) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t n4 = VEC ? n >> 2 : 0;
    for (uint64_t q = first; q < n4; q += stride) {
        const float4 a = stream_load(reinterpret_cast<const float4*>(v) + q);
        const auto word = [&](float f) { return (uint32_t)cs::step_of(f, origin, inv_res); };
        reinterpret_cast<uint4*>(words)[q] = make_uint4(word(a.x), word(a.y), word(a.z), word(a.w));
    }
    for (uint64_t i = (n4 << 2) + first; i < n; i += stride) words[i] = (uint32_t)cs::step_of(v[i], origin, inv_res);
}

// What an LDS cell's two words hold, decoded into the three addends of the planes.
struct StatSums {
    uint32_t n;
    u64 s1, s2;                                                    // sum q (two's complement), sum q^2
};
__device__ __forceinline__ StatSums decode(u64 a, u64 b) {
    constexpr u64 Q = (u64)cs::kQ;
    StatSums r;
    const u64 cnt = a >> kCountShift, su = a & kSumMask;
    r.n = (uint32_t)cnt;
    r.s1 = su - cnt * Q;
    r.s2 = b - 2 * Q * su + cnt * (Q * Q);
    return r;
}

// One work item's records folded into an LDS tile, then merged into the planes.  lds[0 .. cells) = word A, lds[cells .. 2 cells)
// = word B.
__global__ void __launch_bounds__(kThreads)
k_tile_stats(GridDev g, BinGeom b, uint32_t* __restrict__ pn, u64* __restrict__ ps1, u64* __restrict__ ps2,
             const uint2* __restrict__ records, const BinItem* __restrict__ items, const unsigned* __restrict__ n_items) {
    extern __shared__ __align__(16) u64 lds_stat_tile[];
    if (blockIdx.x >= *n_items) return;
    const BinItem it = items[blockIdx.x];
    const int cells = b.tile_w * b.tile_h;                        // a multiple of 1024
    u64* const wa = lds_stat_tile;
    u64* const wb = lds_stat_tile + cells;

    constexpr int kUnroll = 4;
    const uint2* rec = records + it.first;
    uint2 cur[kUnroll], nxt[kUnroll];
    auto fetch = [&](uint2 (&r)[kUnroll], unsigned j0) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const unsigned j = j0 + u * kThreads;
            r[u] = j < it.count ? stream_load(rec + j) : make_uint2(0u, (uint32_t)cs::kNoStep);
        }
    };
    fetch(cur, threadIdx.x);
    for (int i = threadIdx.x; i < cells; i += kThreads)           // (2 cells words of 8 bytes = cells stores of 16)
        reinterpret_cast<uint4*>(lds_stat_tile)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    for (unsigned j0 = threadIdx.x; j0 < it.count; j0 += kUnroll * kThreads) {
        fetch(nxt, j0 + kUnroll * kThreads);                       // past the end: sentinels, no loads issued
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const unsigned c = cur[u].x;
            if (c >= (unsigned)cells || cur[u].y == (uint32_t)cs::kNoStep) continue;
            const u64 uq = (u64)(uint32_t)((int32_t)cur[u].y + cs::kQ);          // in [0, 2^22]
            atomicAdd(&wa[c], ((u64)1 << kCountShift) + uq);
            atomicAdd(&wb[c], uq * uq);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) cur[u] = nxt[u];
    }
    __syncthreads();

    const int bx = it.bin % b.bins_x, by = it.bin / b.bins_x;
    const int c0 = bx * b.tile_w, r0 = b.row0 + by * b.tile_h;     // r0 relative to the state window
    const int w = min(b.tile_w, g.W - c0), h = min(b.tile_h, b.row0 + b.rows - r0);
    if (w <= 0 || h <= 0) return;
    const bool vec = !it.shared && (g.W % 4 == 0) && (w % 4 == 0) &&
                     ((reinterpret_cast<uintptr_t>(pn) | reinterpret_cast<uintptr_t>(ps1) | reinterpret_cast<uintptr_t>(ps2)) & 15) == 0;
    if (vec) {
        const int quads = b.tile_w >> 2, per = quads * h;          // one lane = 4 consecutive cells of a row
        for (int i = threadIdx.x; i < per; i += kThreads) {
            const int ly = i / quads, lx = (i - ly * quads) << 2;
            if (lx >= w) continue;
            const int lc = ly * b.tile_w + lx;
            const ulonglong2 a01 = *reinterpret_cast<const ulonglong2*>(wa + lc), a23 = *reinterpret_cast<const ulonglong2*>(wa + lc + 2);
            if (!((a01.x | a01.y | a23.x | a23.y) >> kCountShift)) continue;      // no cell of the four saw a record
            const ulonglong2 b01 = *reinterpret_cast<const ulonglong2*>(wb + lc), b23 = *reinterpret_cast<const ulonglong2*>(wb + lc + 2);
            const StatSums s0 = decode(a01.x, b01.x), s1 = decode(a01.y, b01.y), s2 = decode(a23.x, b23.x), s3 = decode(a23.y, b23.y);
            const int64_t cell = (int64_t)(r0 + ly) * g.W + (c0 + lx);
            uint4* dn = reinterpret_cast<uint4*>(pn + cell);
            ulonglong2* d1 = reinterpret_cast<ulonglong2*>(ps1 + cell);
            ulonglong2* d2 = reinterpret_cast<ulonglong2*>(ps2 + cell);
            uint4 vn = *dn;
            ulonglong2 p0 = d1[0], p1 = d1[1], q0 = d2[0], q1 = d2[1];
            vn.x += s0.n; vn.y += s1.n; vn.z += s2.n; vn.w += s3.n;
            p0.x += s0.s1; p0.y += s1.s1; p1.x += s2.s1; p1.y += s3.s1;
            q0.x += s0.s2; q0.y += s1.s2; q1.x += s2.s2; q1.y += s3.s2;
            *dn = vn;
            d1[0] = p0; d1[1] = p1;
            d2[0] = q0; d2[1] = q1;
        }
        return;
    }
    const int per = b.tile_w * h;                                  // one lane per cell
    for (int i = threadIdx.x; i < per; i += kThreads) {
        const int ly = i / b.tile_w, lx = i - ly * b.tile_w;
        if (lx >= w) continue;
        const int lc = ly * b.tile_w + lx;
        const u64 a = wa[lc];
        if (!(a >> kCountShift)) continue;
        const StatSums s = decode(a, wb[lc]);
        const int64_t cell = (int64_t)(r0 + ly) * g.W + (c0 + lx);
        if (it.shared) {                                           // other items fold into the same cells
            atomicAdd(pn + cell, s.n);
            atomicAdd(ps1 + cell, s.s1);
            atomicAdd(ps2 + cell, s.s2);
        } else {
            pn[cell] += s.n;
            ps1[cell] += s.s1;
            ps2[cell] += s.s2;
        }
    }
}

// The tile shape: 128 columns x as many rows (a multiple of 8) as fit ~150 KB of the CU's LDS at 16 bytes per cell -- 72 rows,
// 144 KB -- and the device's per-workgroup limit.  tile_h = 0: no fit.
BinGeom stat_bin_geom(const pcr_hip_engine* e) {
    const GridDev& g = e->gd;
    BinGeom b{};
    b.tile_w = kStatTileW;
    b.bins_x = (g.W + b.tile_w - 1) / b.tile_w;
    const size_t row_bytes = (size_t)kStatCellBytes * kStatTileW;
    int h = (int)(std::min<size_t>((size_t)150 * 1024, e->lds_limit) / row_bytes) & ~7;
    h = std::min(h, (1 << kLcellBits) / kStatTileW);
    b.tile_h = h;
    if (h < 8) return b;
    b.bins_y = (g.st_rows + b.tile_h - 1) / b.tile_h;
    b.nbins = b.bins_x * b.bins_y;
    b.rows = g.st_rows;
    return b;
}

struct StatBandArgs {
    int product[cs::kMaxProducts];
    float* out[cs::kMaxProducts];
};

// One lane per cell of the owned rows: the three planes read coalesced, every requested band stored.
__global__ void __launch_bounds__(kBlock)
k_stat_bands(int W, int own_rows, int row_off, const uint32_t* __restrict__ pn, const long long* __restrict__ ps1,
             const u64* __restrict__ ps2, double origin, double resolution, double res2, int ddof, int n_products, StatBandArgs a) {
    const int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= (int64_t)own_rows * W) return;
    const int64_t src = (int64_t)row_off * W + cell;
    float band[cs::kMaxProducts];
    cs::bands_of(pn[src], (int64_t)ps1[src], (uint64_t)ps2[src], origin, resolution, res2, ddof, band[cs::kMean], band[cs::kVariance],
                 band[cs::kStdDev]);
#pragma unroll
    for (int j = 0; j < cs::kMaxProducts; ++j)
        if (j < n_products)
            a.out[j][cell] = a.product[j] == cs::kMean ? band[cs::kMean] : a.product[j] == cs::kVariance ? band[cs::kVariance] : band[cs::kStdDev];
}

int check_band_args(const pcr_hip_grid* g, const void* pn, const void* ps1, const void* ps2, double origin, double resolution, int ddof,
                    int n_products, const int* products, float* const* outs) {
    PCR_REQUIRE(g && pn && ps1 && ps2 && products && outs, "cell_stats_bands: null argument");
    if (int rc = validate_grid(g)) return rc;
    PCR_REQUIRE(std::isfinite(origin) && std::isfinite(resolution) && resolution > 0.0,
                "cell_stats_bands: origin and resolution must be finite, the resolution positive");
    PCR_REQUIRE(ddof == 0 || ddof == 1, "cell_stats_bands: ddof must be 0 or 1");
    PCR_REQUIRE(n_products >= 1 && n_products <= cs::kMaxProducts, "cell_stats_bands: between 1 and 3 products per call");
    for (int j = 0; j < n_products; ++j) {
        PCR_REQUIRE(outs[j], "cell_stats_bands: null output band");
        PCR_REQUIRE(products[j] == cs::kMean || products[j] == cs::kVariance || products[j] == cs::kStdDev,
                    "cell_stats_bands: a product must be 0 (mean), 1 (variance) or 2 (standard deviation)");
    }
    return PCR_HIP_OK;
}

}  // namespace

namespace pcrhip {

int direct_cell_stats(pcr_hip_engine* e, uint32_t* pn, long long* ps1, unsigned long long* ps2, double origin, double inv_res,
                      const double* x, const double* y, const float* v, uint64_t n) {
    const uint64_t want = (n + kBlock - 1) / kBlock;
    const int blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)8 * e->num_cus));
    ScopedKernelTimer t(e, "k_stat_direct");
    hipLaunchKernelGGL(k_stat_direct, dim3(blocks), dim3(kBlock), 0, e->stream, e->gd, pn, reinterpret_cast<u64*>(ps1), ps2, origin,
                       inv_res, x, y, v, n, e->d_touched, e->d_counters);
    PCR_HIP_TRY(hipGetLastError());
    e->stats.path = 0;
    return PCR_HIP_OK;
}

bool binned_cell_stats_supported(const pcr_hip_engine* e) {
    const BinGeom whole = stat_bin_geom(e);
    if (whole.tile_h < 8 || sweep_passes(e, whole) < 1) return false;
    return binned_point_supported(e, PCR_HIP_PLANE_WGT);          // the Point path's own limits: points per call, points per cell
}

int binned_cell_stats(pcr_hip_engine* e, uint32_t* pn, long long* ps1, unsigned long long* ps2, double origin, double inv_res,
                      const double* x, const double* y, const float* v, uint64_t n) {
    const BinGeom whole = stat_bin_geom(e);
    // the step words: the grow-only buffer of the engine's own that the histogram's bin words use (one scatter at a time is in
    // the making, and the stream orders their uses)
    if (e->hist_words_cap < n) {
        PCR_HIP_TRY(hipStreamSynchronize(e->stream));             // (an earlier scatter may still read the old block)
        if (e->d_hist_words) (void)hipFree(e->d_hist_words);
        e->d_hist_words = nullptr;
        e->hist_words_cap = 0;
        const size_t cap = (size_t)(n + n / 8 + 1024);
        PCR_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&e->d_hist_words), cap * sizeof(uint32_t)));
        e->hist_words_cap = cap;
    }
    {
        ScopedKernelTimer t(e, "k_stat_steps");
        const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)8 * e->num_cus));
        if ((reinterpret_cast<uintptr_t>(v) & 15) == 0)
            hipLaunchKernelGGL(k_stat_steps<true>, dim3(blocks), dim3(kBlock), 0, e->stream, v, e->d_hist_words, n, origin, inv_res);
        else
            hipLaunchKernelGGL(k_stat_steps<false>, dim3(blocks), dim3(kBlock), 0, e->stream, v, e->d_hist_words, n, origin, inv_res);
    }
    const int visited = sweep_tiles(e, whole, x, y, reinterpret_cast<const float*>(e->d_hist_words), n, RecordKind::Value,
                                    kStatItemRecords, false, 0, [&](const GridDev& gd, const BinGeom& b, const BinBuffers& bb) {
        ScopedKernelTimer t(e, "k_tile_stats");
        const size_t lds = (size_t)kStatCellBytes * b.tile_w * b.tile_h;
        allow_dynamic_lds(e, reinterpret_cast<const void*>(&k_tile_stats), lds);
        hipLaunchKernelGGL(k_tile_stats, dim3(bb.max_items), dim3(kThreads), lds, e->stream, gd, b, pn, reinterpret_cast<u64*>(ps1), ps2,
                           bb.records, bb.items, bb.n_items);
        return (int)PCR_HIP_OK;
    });
    if (visited < 0) return -visited;
    PCR_HIP_TRY(hipGetLastError());
    set_binned_stats(e, 1, whole.tile_w, whole.tile_h, 0, visited);
    return PCR_HIP_OK;
}

}  // namespace pcrhip

extern "C" {

int pcr_hip_cell_stats_bands(const pcr_hip_grid* g, const uint32_t* d_n, const long long* d_s1, const unsigned long long* d_s2,
                             double origin, double resolution, int ddof, int n_products, const int* products, float* const* d_outs,
                             pcr_hip_stream s) {
    if (int rc = check_band_args(g, d_n, d_s1, d_s2, origin, resolution, ddof, n_products, products, d_outs)) return rc;
    const int own_rows = g->own_row1 - g->own_row0;
    if (own_rows <= 0) return PCR_HIP_OK;
    StatBandArgs a{};
    for (int j = 0; j < n_products; ++j) { a.product[j] = products[j]; a.out[j] = d_outs[j]; }
    const int64_t cells = (int64_t)own_rows * g->width;
    const unsigned blocks = (unsigned)((cells + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_stat_bands, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(s), g->width, own_rows,
                       g->own_row0 - g->state_row0, d_n, d_s1, d_s2, origin, resolution, resolution * resolution, ddof, n_products, a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_cell_stats_bands_host(const pcr_hip_grid* g, const uint32_t* h_n, const long long* h_s1, const unsigned long long* h_s2,
                                  double origin, double resolution, int ddof, int n_products, const int* products, float* const* h_outs) {
    if (int rc = check_band_args(g, h_n, h_s1, h_s2, origin, resolution, ddof, n_products, products, h_outs)) return rc;
    const int own_rows = g->own_row1 - g->own_row0, W = g->width;
    const int64_t cells = (int64_t)std::max(own_rows, 0) * W, off = (int64_t)(g->own_row0 - g->state_row0) * W;
    const double res2 = resolution * resolution;
    for (int64_t cell = 0; cell < cells; ++cell) {
        float band[cs::kMaxProducts];
        cs::bands_of(h_n[off + cell], (int64_t)h_s1[off + cell], (uint64_t)h_s2[off + cell], origin, resolution, res2, ddof, band[cs::kMean],
                     band[cs::kVariance], band[cs::kStdDev]);
        for (int j = 0; j < n_products; ++j) h_outs[j][cell] = band[products[j]];
    }
    return PCR_HIP_OK;
}

}  // extern "C"
