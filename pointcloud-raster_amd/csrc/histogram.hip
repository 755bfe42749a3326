// histogram.hip -- per-cell value histograms (the contract: histogram.hpp, include/pcr_hip.h "per-cell histograms"): the two
// scatter paths behind pcr_hip_scatter_histogram, and pcr_hip_histogram_percentiles with its host twin.
//
// State: a cube of `bins` planes of uint32 counters in the state window's layout, count[b][cell].  The fold is integer
// addition, so every path, order and chunking gives the same bits.
//   direct   k_hist_direct: route + one no-return 32-bit global atomic add per accepted point.
//   binned   the Point front end unchanged (k_bin_count, k_bin_scan, k_bin_scatter in all their forms, through sweep_tiles),
//            as MostRecent uses it, but with nothing to gather: a streaming pre-pass (k_hist_bins) turns every value into
//            one 32-bit word, its bin index (kNoBin for a NaN), and that word rides through the scatter pass in the VALUE
//            slot of ordinary 8-byte records {local cell, bin}.  The tile pass (k_tile_hist) then needs the records alone.
//            An LDS tile is 128 x h cells x S consecutive bins of uint32 (ds_add_u32); with more bins than S the records
//            are sorted ONCE and the tile pass is launched ceil(bins / S) times over them, launch s folding the records
//            whose bin lies in slab s (a record re-read is 8 streamed bytes).
#include "engine.hpp"
#include "histogram.hpp"

#include <algorithm>
#include <cmath>

using namespace pcrhip;

namespace {

constexpr int kBlock = 256;
constexpr int kThreads = 1024;                    // full-CU workgroups, as the Point tile pass
constexpr int kHistTileW = 128;                   // a row of one bin plane of a tile: a contiguous 512-byte run
// A bin with more records than this is split into several work items, which then merge with atomics.  Half of the Point
// pass's: an item here costs its records ceil(bins / S) times over, and the zeroing and the merge of 128 KB of LDS each time.
constexpr unsigned kHistItemRecords = 1u << 16;

// ---- direct path -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_hist_direct(GridDev g, uint32_t* __restrict__ counts, int64_t plane_cells, int bins, double lo, double inv_w,
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
            const uint32_t b = hist::bin_of(v[i], lo, inv_w, bins);
            if (b != hist::kNoBin)                                // (the result is unused: global_atomic_add_u32 without return)
                atomicAdd(counts + (int64_t)b * plane_cells + ((int64_t)(row - g.st_r0) * g.W + col), 1u);
            touch_tile(g, touched, row, col);
        }
        const unsigned long long m = __ballot(valid);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(counters, (unsigned long long)__popcll(m));
    }
}

// ---- binned path -----------------------------------------------------------------------------------------------------------
// words[i] = bin of v[i], kNoBin for a NaN: 4 B read and 4 B written per point, streaming.  VEC: four points per lane.
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
k_hist_bins(const float* __restrict__ v, uint32_t* __restrict__ words, uint64_t n, int bins, double lo, double inv_w) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t n4 = VEC ? n >> 2 : 0;
    for (uint64_t q = first; q < n4; q += stride) {
        const float4 a = stream_load(reinterpret_cast<const float4*>(v) + q);
        reinterpret_cast<uint4*>(words)[q] = make_uint4(hist::bin_of(a.x, lo, inv_w, bins), hist::bin_of(a.y, lo, inv_w, bins),
                                                        hist::bin_of(a.z, lo, inv_w, bins), hist::bin_of(a.w, lo, inv_w, bins));
    }
    for (uint64_t i = (n4 << 2) + first; i < n; i += stride) words[i] = hist::bin_of(v[i], lo, inv_w, bins);
}

// One work item's records folded into an LDS tile of `ns` bin planes (bins [slab0, slab0 + ns)), then merged into the cube.
// lds[s * cells + local cell].  A record of another slab, or of a NaN value (kNoBin), fails the one unsigned comparison.
// Merge: an exclusively owned bin adds its non-zero counters into the cube with plain 16-byte read-modify-writes (a row of
// a bin plane is a contiguous run); a bin the scan split (it.shared) uses the global atomic add.  The cube is zero at create
// and only ever added to: there is no "fresh" form.
__global__ void __launch_bounds__(kThreads)
k_tile_hist(GridDev g, BinGeom b, uint32_t* __restrict__ counts, int64_t plane_cells, int slab0, int ns,
            const uint2* __restrict__ records, const BinItem* __restrict__ items, const unsigned* __restrict__ n_items) {
    extern __shared__ unsigned lds_hist_tile[];
    if (blockIdx.x >= *n_items) return;
    const BinItem it = items[blockIdx.x];
    const int cells = b.tile_w * b.tile_h;                        // a multiple of 1024

    constexpr int kUnroll = 4;
    const uint2* rec = records + it.first;
    uint2 cur[kUnroll], nxt[kUnroll];
    auto fetch = [&](uint2 (&r)[kUnroll], unsigned j0) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const unsigned j = j0 + u * kThreads;
            r[u] = j < it.count ? stream_load(rec + j) : make_uint2(0u, hist::kNoBin);
        }
    };
    fetch(cur, threadIdx.x);
    for (int i = threadIdx.x; i < (ns * cells) >> 2; i += kThreads) reinterpret_cast<uint4*>(lds_hist_tile)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();

    for (unsigned j0 = threadIdx.x; j0 < it.count; j0 += kUnroll * kThreads) {
        fetch(nxt, j0 + kUnroll * kThreads);                       // past the end: sentinels, no loads issued
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const unsigned rel = cur[u].y - (unsigned)slab0;       // wraps for a lower slab and for kNoBin
            if (rel < (unsigned)ns && cur[u].x < (unsigned)cells) atomicAdd(&lds_hist_tile[rel * (unsigned)cells + cur[u].x], 1u);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) cur[u] = nxt[u];
    }
    __syncthreads();

    const int bx = it.bin % b.bins_x, by = it.bin / b.bins_x;
    const int c0 = bx * b.tile_w, r0 = b.row0 + by * b.tile_h;     // r0 relative to the state window
    const int w = min(b.tile_w, g.W - c0), h = min(b.tile_h, b.row0 + b.rows - r0);
    const bool vec = !it.shared && (g.W % 4 == 0) && (w % 4 == 0) && (reinterpret_cast<uintptr_t>(counts) & 15) == 0;
    if (vec) {
        const int quads = b.tile_w >> 2, per = quads * h;          // one lane = 4 consecutive cells of a row = 16 bytes
        for (int i = threadIdx.x; i < ns * per; i += kThreads) {
            const int s = i / per, k = i - s * per;
            const int ly = k / quads, lx = (k - ly * quads) << 2;
            if (lx >= w) continue;
            const uint4 a = *reinterpret_cast<const uint4*>(lds_hist_tile + s * cells + ly * b.tile_w + lx);
            if (!(a.x | a.y | a.z | a.w)) continue;
            uint4* dst = reinterpret_cast<uint4*>(counts + (int64_t)(slab0 + s) * plane_cells + ((int64_t)(r0 + ly) * g.W + (c0 + lx)));
            uint4 c = *dst;
            c.x += a.x; c.y += a.y; c.z += a.z; c.w += a.w;
            *dst = c;
        }
        return;
    }
    const int per = b.tile_w * h;
    for (int i = threadIdx.x; i < ns * per; i += kThreads) {
        const int s = i / per, k = i - s * per;
        const int ly = k / b.tile_w, lx = k - ly * b.tile_w;
        if (lx >= w) continue;
        const unsigned a = lds_hist_tile[s * cells + ly * b.tile_w + lx];
        if (!a) continue;
        uint32_t* dst = counts + (int64_t)(slab0 + s) * plane_cells + ((int64_t)(r0 + ly) * g.W + (c0 + lx));
        if (it.shared) atomicAdd(dst, a);
        else *dst += a;
    }
}

// The tile shape for S bin planes per tile: 128 columns x as many rows (a multiple of 8) as fit ~150 KB of the CU's LDS at
// 4 S bytes per cell -- 32, 16 and 8 rows at S = 8, 16 and 32 -- and the device's per-workgroup limit.  tile_h = 0: no fit.
BinGeom hist_bin_geom(const pcr_hip_engine* e, int S) {
    const GridDev& g = e->gd;
    BinGeom b{};
    b.tile_w = kHistTileW;
    b.bins_x = (g.W + b.tile_w - 1) / b.tile_w;
    const size_t row_bytes = (size_t)4 * S * kHistTileW;
    int h = (int)(std::min<size_t>((size_t)150 * 1024, e->lds_limit) / row_bytes) & ~7;
    h = std::min(h, (1 << kLcellBits) / kHistTileW);
    b.tile_h = h;
    if (h < 8) return b;
    b.bins_y = (g.st_rows + b.tile_h - 1) / b.tile_h;
    b.nbins = b.bins_x * b.bins_y;
    b.rows = g.st_rows;
    return b;
}

struct PercentileArgs {
    float q[hist::kMaxPercentiles];
    float* out[hist::kMaxPercentiles];
};

// One lane per cell of the owned rows; the bin planes are read coalesced, twice at most: the total, then the walk, which
// serves every band of the histogram and ends at the bin that holds the greatest rank.
__global__ void __launch_bounds__(kBlock)
k_hist_percentiles(int W, int own_rows, int row_off, const uint32_t* __restrict__ counts, int64_t plane_cells, int bins, double lo,
                   double w, int n_q, PercentileArgs a) {
    const int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (cell >= (int64_t)own_rows * W) return;
    const uint32_t* mine = counts + (int64_t)row_off * W + cell;
    uint64_t total = 0;
    for (int b = 0; b < bins; ++b) total += mine[(int64_t)b * plane_cells];
    if (total == 0) {
        for (int j = 0; j < n_q; ++j) a.out[j][cell] = hist::nodata();
        return;
    }
    int64_t k[hist::kMaxPercentiles];
    int64_t k_max = 0;
#pragma unroll
    for (int j = 0; j < hist::kMaxPercentiles; ++j) {
        k[j] = j < n_q ? hist::rank_of(a.q[j], total) : 0;
        k_max = k[j] > k_max ? k[j] : k_max;
    }
    uint64_t below = 0;
    for (int b = 0; b < bins && (int64_t)below < k_max; ++b) {
        const uint32_t c = mine[(int64_t)b * plane_cells];
        const uint64_t upto = below + c;
#pragma unroll
        for (int j = 0; j < hist::kMaxPercentiles; ++j)
            if (j < n_q && k[j] > (int64_t)below && k[j] <= (int64_t)upto) a.out[j][cell] = hist::value_at(lo, w, b, k[j], below, c);
        below = upto;
    }
}

int check_percentile_args(const pcr_hip_grid* g, const uint32_t* counts, int bins, double lo, double w, int n_q, const float* q,
                          float* const* outs) {
    PCR_REQUIRE(g && counts && q && outs, "histogram_percentiles: null argument");
    if (int rc = validate_grid(g)) return rc;
    PCR_REQUIRE(bins >= 1 && bins <= hist::kMaxBins, "histogram_percentiles: bins must be between 1 and 256");
    PCR_REQUIRE(n_q >= 1 && n_q <= hist::kMaxPercentiles, "histogram_percentiles: between 1 and 16 percentiles per call");
    PCR_REQUIRE(std::isfinite(lo) && std::isfinite(w) && w > 0.0, "histogram_percentiles: lo and the bin width must be finite, the width positive");
    for (int j = 0; j < n_q; ++j) {
        PCR_REQUIRE(outs[j], "histogram_percentiles: null output band");
        PCR_REQUIRE(q[j] >= 0.0f && q[j] <= 1.0f, "histogram_percentiles: a percentile must lie in [0, 1]");
    }
    return PCR_HIP_OK;
}

}  // namespace

namespace pcrhip {

int direct_hist(pcr_hip_engine* e, uint32_t* counts, int bins, double lo, double inv_w, const double* x, const double* y,
                const float* v, uint64_t n) {
    const uint64_t want = (n + kBlock - 1) / kBlock;
    const int blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)8 * e->num_cus));
    ScopedKernelTimer t(e, "k_hist_direct");
    hipLaunchKernelGGL(k_hist_direct, dim3(blocks), dim3(kBlock), 0, e->stream, e->gd, counts, (int64_t)e->gd.st_rows * e->gd.W, bins,
                       lo, inv_w, x, y, v, n, e->d_touched, e->d_counters);
    PCR_HIP_TRY(hipGetLastError());
    e->stats.path = 0;
    return PCR_HIP_OK;
}

bool binned_hist_supported(const pcr_hip_engine* e) {
    const BinGeom whole = hist_bin_geom(e, e->hist_slab);
    if (whole.tile_h < 8 || sweep_passes(e, whole) < 1) return false;
    return binned_point_supported(e, PCR_HIP_PLANE_WGT);          // the Point path's own limits: points per call, points per cell
}

int binned_hist(pcr_hip_engine* e, uint32_t* counts, int bins, double lo, double inv_w, const double* x, const double* y,
                const float* v, uint64_t n) {
    const int S = e->hist_slab;
    const BinGeom whole = hist_bin_geom(e, S);
    // the bin words: a buffer of the engine's own, grow-only (the scratch arena is carved anew by every pass of the sweep)
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
        ScopedKernelTimer t(e, "k_hist_bins");
        const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)8 * e->num_cus));
        if ((reinterpret_cast<uintptr_t>(v) & 15) == 0)
            hipLaunchKernelGGL(k_hist_bins<true>, dim3(blocks), dim3(kBlock), 0, e->stream, v, e->d_hist_words, n, bins, lo, inv_w);
        else
            hipLaunchKernelGGL(k_hist_bins<false>, dim3(blocks), dim3(kBlock), 0, e->stream, v, e->d_hist_words, n, bins, lo, inv_w);
    }
    const int64_t plane_cells = (int64_t)e->gd.st_rows * e->gd.W;
    const int visited = sweep_tiles(e, whole, x, y, reinterpret_cast<const float*>(e->d_hist_words), n, RecordKind::Value,
                                    kHistItemRecords, false, 0, [&](const GridDev& gd, const BinGeom& b, const BinBuffers& bb) {
        ScopedKernelTimer t(e, "k_tile_hist");
        for (int slab0 = 0; slab0 < bins; slab0 += S) {
            const int ns = std::min(S, bins - slab0);
            const size_t lds = (size_t)ns * b.tile_w * b.tile_h * sizeof(uint32_t);
            allow_dynamic_lds(e, reinterpret_cast<const void*>(&k_tile_hist), lds);
            hipLaunchKernelGGL(k_tile_hist, dim3(bb.max_items), dim3(kThreads), lds, e->stream, gd, b, counts, plane_cells, slab0, ns,
                               bb.records, bb.items, bb.n_items);
        }
        return (int)PCR_HIP_OK;
    });
    if (visited < 0) return -visited;
    PCR_HIP_TRY(hipGetLastError());
    set_binned_stats(e, 1, whole.tile_w, whole.tile_h, 0, visited);
    return PCR_HIP_OK;
}

}  // namespace pcrhip

extern "C" {

int pcr_hip_histogram_percentiles(const pcr_hip_grid* g, const uint32_t* d_counts, int bins, double lo, double w, int n_q,
                                  const float* q, float* const* d_outs, pcr_hip_stream s) {
    if (int rc = check_percentile_args(g, d_counts, bins, lo, w, n_q, q, d_outs)) return rc;
    const int own_rows = g->own_row1 - g->own_row0;
    if (own_rows <= 0) return PCR_HIP_OK;
    PercentileArgs a{};
    for (int j = 0; j < n_q; ++j) { a.q[j] = q[j]; a.out[j] = d_outs[j]; }
    const int64_t cells = (int64_t)own_rows * g->width;
    const unsigned blocks = (unsigned)((cells + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_hist_percentiles, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(s), g->width, own_rows,
                       g->own_row0 - g->state_row0, d_counts, (int64_t)g->state_rows * g->width, bins, lo, w, n_q, a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_histogram_percentiles_host(const pcr_hip_grid* g, const uint32_t* h_counts, int bins, double lo, double w, int n_q,
                                       const float* q, float* const* h_outs) {
    if (int rc = check_percentile_args(g, h_counts, bins, lo, w, n_q, q, h_outs)) return rc;
    const int own_rows = g->own_row1 - g->own_row0, W = g->width;
    const int64_t plane_cells = (int64_t)g->state_rows * W, cells = (int64_t)std::max(own_rows, 0) * W;
    const uint32_t* base = h_counts + (int64_t)(g->own_row0 - g->state_row0) * W;
    for (int64_t cell = 0; cell < cells; ++cell) {
        const uint32_t* mine = base + cell;
        uint64_t total = 0;
        for (int b = 0; b < bins; ++b) total += mine[(int64_t)b * plane_cells];
        if (total == 0) {
            for (int j = 0; j < n_q; ++j) h_outs[j][cell] = hist::nodata();
            continue;
        }
        int64_t k[hist::kMaxPercentiles], k_max = 0;
        for (int j = 0; j < n_q; ++j) {
            k[j] = hist::rank_of(q[j], total);
            k_max = std::max(k_max, k[j]);
        }
        uint64_t below = 0;
        for (int b = 0; b < bins && (int64_t)below < k_max; ++b) {
            const uint32_t c = mine[(int64_t)b * plane_cells];
            const uint64_t upto = below + c;
            for (int j = 0; j < n_q; ++j)
                if (k[j] > (int64_t)below && k[j] <= (int64_t)upto) h_outs[j][cell] = hist::value_at(lo, w, b, k[j], below, c);
            below = upto;
        }
    }
    return PCR_HIP_OK;
}

}  // extern "C"
