// extremes.hip -- per-cell extremes (the contract: extremes.hpp, include/pcr_hip.h "per-cell extremes"): the two scatter paths
// behind pcr_hip_scatter_extremes, and pcr_hip_extremes_band with its host twin.
//
// State: k planes of uint32 keys in the state window's layout, keys[j][cell], all kEmpty at create; plane j of a cell holds the
// (j+1)-th smallest distinct key among the cell's accepted points.  The k smallest distinct keys of a set do not depend on the
// order the set is presented in, so every path, order and chunking gives the same bits.
//   the chain  insert(key): at slot j, old = atomicMin(&slot[j], key); stop if old == key (a duplicate); else carry
//              max(old, key) to slot j + 1; stop when the carried key is kEmpty or j + 1 == k.  Slots only ever decrease; slot 0
//              ends as the minimum of everything, slot 1 as the minimum of everything that was passed on, and so on.  A key >=
//              the current slot[k-1] can never enter (the slot only decreases): one read ends most records without an atomic.
//   direct     k_ext_direct: route, key, the chain with returning 32-bit global atomics.
//   binned     the Point front end unchanged (through sweep_tiles), as the histogram uses it: a streaming pre-pass (k_ext_keys)
//              turns every value into its key word (kEmpty for a NaN), and that word rides through the scatter pass in the VALUE
//              slot of ordinary 8-byte records {local cell, key}.  The tile pass (k_tile_extremes) runs the chain with LDS
//              atomics on a tile of 128 x h cells x k planes, PLANE-MAJOR (lds[j * cells + cell]): the records of a tile hit
//              random cells, so the 64 lanes of the early-out read (plane k-1) and of the first atomic (plane 0) spread over all
//              the banks as cell % 64 does; interleaved per cell those two accesses would use only every k-th bank, a k-way
//              conflict on the two instructions nearly every record executes.  Plane-major rows are also contiguous 512-byte
//              runs, which the merge reads 16 bytes wide.  Merge: an exclusively owned item merges each cell's sorted LDS list
//              into the cell's sorted global list with plain reads and writes; an item the scan split runs the chain with global
//              atomics for every LDS key.
#include "engine.hpp"
#include "extremes.hpp"

#include <algorithm>
#include <cmath>

using namespace pcrhip;

namespace {

constexpr int kBlock = 256;
constexpr int kThreads = 1024;                    // full-CU workgroups, as the Point tile pass
constexpr int kExtTileW = 128;                    // a row of one key plane of a tile: a contiguous 512-byte run
// A bin with more records than this is split into several work items, which then merge with atomics (as the histogram's).
constexpr unsigned kExtItemRecords = 1u << 16;

__device__ __forceinline__ uint32_t load_global(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t load_lds(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// The chain on the k global slots of one cell, `stride` words apart.
__device__ __forceinline__ void chain_global(uint32_t* slot, int64_t stride, int k, uint32_t key) {
    if (key >= load_global(slot + (int64_t)(k - 1) * stride)) return;   // (also a NaN's kEmpty)
    uint32_t carry = key;
    for (int j = 0; j < k; ++j) {
        const uint32_t old = atomicMin(slot + (int64_t)j * stride, carry);
        if (old == carry) return;
        carry = old > carry ? old : carry;
        if (carry == ext::kEmpty) return;
    }
}

// ---- direct path -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_ext_direct(GridDev g, uint32_t* __restrict__ keys, int64_t plane_cells, int k, int side, const double* __restrict__ x,
             const double* __restrict__ y, const float* __restrict__ v, uint64_t n, uint32_t* __restrict__ touched,
             unsigned long long* __restrict__ counters) {
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
            chain_global(keys + ((int64_t)(row - g.st_r0) * g.W + col), plane_cells, k, ext::key_of(v[i], side));
            touch_tile(g, touched, row, col);
        }
        const unsigned long long m = __ballot(valid);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(counters, (unsigned long long)__popcll(m));
    }
}

// ---- binned path -----------------------------------------------------------------------------------------------------------
// words[i] = key of v[i], kEmpty for a NaN: 4 B read and 4 B written per point, streaming.  VEC: four points per lane.
template <bool VEC>
__global__ void __launch_bounds__(kBlock)
k_ext_keys(const float* __restrict__ v, uint32_t* __restrict__ words, uint64_t n, int side) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    const uint64_t first = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t n4 = VEC ? n >> 2 : 0;
    for (uint64_t q = first; q < n4; q += stride) {
        const float4 a = stream_load(reinterpret_cast<const float4*>(v) + q);
        reinterpret_cast<uint4*>(words)[q] = make_uint4(ext::key_of(a.x, side), ext::key_of(a.y, side), ext::key_of(a.z, side),
                                                        ext::key_of(a.w, side));
    }
    for (uint64_t i = (n4 << 2) + first; i < n; i += stride) words[i] = ext::key_of(v[i], side);
}

// The chain in registers: `key` into the ascending distinct list g[0..K) of one cell -- what the chain does when one lane owns
// the cell.  Every index is a constant once unrolled.
template <int K>
__device__ __forceinline__ void insert_reg(uint32_t (&g)[K], uint32_t key) {
    uint32_t carry = key;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (carry == g[j]) carry = ext::kEmpty;                    // a duplicate (or nothing left to carry): the rest stays
        const uint32_t lo = g[j] < carry ? g[j] : carry;
        carry = g[j] < carry ? carry : g[j];
        g[j] = lo;
    }
}

// One work item's records folded into an LDS tile of K key planes, then merged into the state.  lds[j * cells + local cell].
template <int K>
__global__ void __launch_bounds__(kThreads)
k_tile_extremes(GridDev g, BinGeom b, uint32_t* __restrict__ keys, int64_t plane_cells, const uint2* __restrict__ records,
                const BinItem* __restrict__ items, const unsigned* __restrict__ n_items) {
    extern __shared__ uint32_t lds_ext_tile[];
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
            r[u] = j < it.count ? stream_load(rec + j) : make_uint2(0u, ext::kEmpty);
        }
    };
    fetch(cur, threadIdx.x);
    for (int i = threadIdx.x; i < (K * cells) >> 2; i += kThreads)
        reinterpret_cast<uint4*>(lds_ext_tile)[i] = make_uint4(ext::kEmpty, ext::kEmpty, ext::kEmpty, ext::kEmpty);
    __syncthreads();

    for (unsigned j0 = threadIdx.x; j0 < it.count; j0 += kUnroll * kThreads) {
        fetch(nxt, j0 + kUnroll * kThreads);                       // past the end: sentinels, no loads issued
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const unsigned c = cur[u].x;
            uint32_t carry = cur[u].y;
            // the early-out: a key at or above the cell's last slot (a NaN's kEmpty always is) can never enter
            if (c >= (unsigned)cells || carry >= load_lds(&lds_ext_tile[(K - 1) * cells + c])) continue;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t old = atomicMin(&lds_ext_tile[j * cells + c], carry);
                if (old == carry) break;
                carry = old > carry ? old : carry;
                if (carry == ext::kEmpty) break;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) cur[u] = nxt[u];
    }
    __syncthreads();

    const int bx = it.bin % b.bins_x, by = it.bin / b.bins_x;
    const int c0 = bx * b.tile_w, r0 = b.row0 + by * b.tile_h;     // r0 relative to the state window
    const int w = min(b.tile_w, g.W - c0), h = min(b.tile_h, b.row0 + b.rows - r0);
    if (w <= 0 || h <= 0) return;
    if (it.shared) {                                               // other items fold into the same cells: the chain, atomically
        const int per = b.tile_w * h;
        for (int i = threadIdx.x; i < per; i += kThreads) {
            const int ly = i / b.tile_w, lx = i - ly * b.tile_w;
            if (lx >= w) continue;
            const int lc = ly * b.tile_w + lx;
            uint32_t* dst = keys + ((int64_t)(r0 + ly) * g.W + (c0 + lx));
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t a = lds_ext_tile[j * cells + lc];
                if (a == ext::kEmpty) break;
                chain_global(dst, plane_cells, K, a);
            }
        }
        return;
    }
    const bool vec = (g.W % 4 == 0) && (w % 4 == 0) && (reinterpret_cast<uintptr_t>(keys) & 15) == 0 && (plane_cells % 4 == 0);
    if (vec) {
        const int quads = b.tile_w >> 2, per = quads * h;          // one lane = 4 consecutive cells of a row = 16 bytes a plane
        for (int i = threadIdx.x; i < per; i += kThreads) {
            const int ly = i / quads, lx = (i - ly * quads) << 2;
            if (lx >= w) continue;
            const int lc = ly * b.tile_w + lx;
            const uint4 a0 = *reinterpret_cast<const uint4*>(lds_ext_tile + lc);
            if ((a0.x & a0.y & a0.z & a0.w) == ext::kEmpty) continue;     // no cell of the four saw a record
            uint32_t* dst = keys + ((int64_t)(r0 + ly) * g.W + (c0 + lx));
            uint32_t gx[K], gy[K], gz[K], gw[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint4 q = *reinterpret_cast<const uint4*>(dst + (int64_t)j * plane_cells);
                gx[j] = q.x; gy[j] = q.y; gz[j] = q.z; gw[j] = q.w;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint4 a = *reinterpret_cast<const uint4*>(lds_ext_tile + j * cells + lc);
                insert_reg<K>(gx, a.x);
                insert_reg<K>(gy, a.y);
                insert_reg<K>(gz, a.z);
                insert_reg<K>(gw, a.w);
            }
#pragma unroll
            for (int j = 0; j < K; ++j) *reinterpret_cast<uint4*>(dst + (int64_t)j * plane_cells) = make_uint4(gx[j], gy[j], gz[j], gw[j]);
        }
        return;
    }
    const int per = b.tile_w * h;
    for (int i = threadIdx.x; i < per; i += kThreads) {
        const int ly = i / b.tile_w, lx = i - ly * b.tile_w;
        if (lx >= w) continue;
        const int lc = ly * b.tile_w + lx;
        if (lds_ext_tile[lc] == ext::kEmpty) continue;
        uint32_t* dst = keys + ((int64_t)(r0 + ly) * g.W + (c0 + lx));
        uint32_t gk[K];
#pragma unroll
        for (int j = 0; j < K; ++j) gk[j] = dst[(int64_t)j * plane_cells];
#pragma unroll
        for (int j = 0; j < K; ++j) insert_reg<K>(gk, lds_ext_tile[j * cells + lc]);
#pragma unroll
        for (int j = 0; j < K; ++j) dst[(int64_t)j * plane_cells] = gk[j];
    }
}

// The tile shape for k key planes per tile: 128 columns x as many rows (a multiple of 8) as fit ~150 KB of the CU's LDS at 4 k
// bytes per cell -- 144, 72 and 32 rows at k = 2, 4 and 8 -- and the device's per-workgroup limit.  tile_h = 0: no fit.
BinGeom ext_bin_geom(const pcr_hip_engine* e, int k) {
    const GridDev& g = e->gd;
    BinGeom b{};
    b.tile_w = kExtTileW;
    b.bins_x = (g.W + b.tile_w - 1) / b.tile_w;
    const size_t row_bytes = (size_t)4 * k * kExtTileW;
    int h = (int)(std::min<size_t>((size_t)150 * 1024, e->lds_limit) / row_bytes) & ~7;
    h = std::min(h, (1 << kLcellBits) / kExtTileW);
    b.tile_h = h;
    if (h < 8) return b;
    b.bins_y = (g.st_rows + b.tile_h - 1) / b.tile_h;
    b.nbins = b.bins_x * b.bins_y;
    b.rows = g.st_rows;
    return b;
}

template <int K>
void launch_tile(pcr_hip_engine* e, const GridDev& gd, const BinGeom& b, const BinBuffers& bb, uint32_t* keys, int64_t plane_cells) {
    const size_t lds = (size_t)K * b.tile_w * b.tile_h * sizeof(uint32_t);
    allow_dynamic_lds(e, reinterpret_cast<const void*>(&k_tile_extremes<K>), lds);
    hipLaunchKernelGGL(k_tile_extremes<K>, dim3(bb.max_items), dim3(kThreads), lds, e->stream, gd, b, keys, plane_cells, bb.records,
                       bb.items, bb.n_items);
}

// One lane per cell of the owned rows: the k planes read coalesced, the walk of extremes.hpp, the band stored -- and, where
// asked, the k decoded values.
__global__ void __launch_bounds__(kBlock)
k_ext_band(int W, int own_rows, int row_off, const uint32_t* __restrict__ keys, int64_t plane_cells, int k, int side, float max_gap,
           float* __restrict__ out, float* __restrict__ values) {
    const int64_t cell = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t own_cells = (int64_t)own_rows * W;
    if (cell >= own_cells) return;
    out[cell] = ext::band_of(keys + (int64_t)row_off * W + cell, plane_cells, k, side, max_gap, values ? values + cell : nullptr, own_cells);
}

int check_band_args(const pcr_hip_grid* g, const uint32_t* keys, int k, int side, float max_gap, const float* out) {
    PCR_REQUIRE(g && keys && out, "extremes_band: null argument");
    if (int rc = validate_grid(g)) return rc;
    PCR_REQUIRE(k >= ext::kMinK && k <= ext::kMaxK, "extremes_band: k must be between 2 and 8");
    PCR_REQUIRE(side == ext::kLowest || side == ext::kHighest, "extremes_band: side must be 0 (lowest) or 1 (highest)");
    PCR_REQUIRE(max_gap >= 0.0f, "extremes_band: max_gap must not be negative or NaN");
    return PCR_HIP_OK;
}

}  // namespace

namespace pcrhip {

int direct_extremes(pcr_hip_engine* e, uint32_t* keys, int k, int side, const double* x, const double* y, const float* v, uint64_t n) {
    const uint64_t want = (n + kBlock - 1) / kBlock;
    const int blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)8 * e->num_cus));
    ScopedKernelTimer t(e, "k_ext_direct");
    hipLaunchKernelGGL(k_ext_direct, dim3(blocks), dim3(kBlock), 0, e->stream, e->gd, keys, (int64_t)e->gd.st_rows * e->gd.W, k, side, x,
                       y, v, n, e->d_touched, e->d_counters);
    PCR_HIP_TRY(hipGetLastError());
    e->stats.path = 0;
    return PCR_HIP_OK;
}

bool binned_extremes_supported(const pcr_hip_engine* e, int k) {
    const BinGeom whole = ext_bin_geom(e, k);
    if (whole.tile_h < 8 || sweep_passes(e, whole) < 1) return false;
    return binned_point_supported(e, PCR_HIP_PLANE_WGT);          // the Point path's own limits: points per call, points per cell
}

int binned_extremes(pcr_hip_engine* e, uint32_t* keys, int k, int side, const double* x, const double* y, const float* v, uint64_t n) {
    const BinGeom whole = ext_bin_geom(e, k);
    // the key words: the grow-only buffer of the engine's own that the histogram's bin words use (one scatter at a time is in
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
        ScopedKernelTimer t(e, "k_ext_keys");
        const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)8 * e->num_cus));
        if ((reinterpret_cast<uintptr_t>(v) & 15) == 0)
            hipLaunchKernelGGL(k_ext_keys<true>, dim3(blocks), dim3(kBlock), 0, e->stream, v, e->d_hist_words, n, side);
        else
            hipLaunchKernelGGL(k_ext_keys<false>, dim3(blocks), dim3(kBlock), 0, e->stream, v, e->d_hist_words, n, side);
    }
    const int64_t plane_cells = (int64_t)e->gd.st_rows * e->gd.W;
    const int visited = sweep_tiles(e, whole, x, y, reinterpret_cast<const float*>(e->d_hist_words), n, RecordKind::Value,
                                    kExtItemRecords, false, 0, [&](const GridDev& gd, const BinGeom& b, const BinBuffers& bb) {
        ScopedKernelTimer t(e, "k_tile_extremes");
        switch (k) {
            case 2: launch_tile<2>(e, gd, b, bb, keys, plane_cells); break;
            case 3: launch_tile<3>(e, gd, b, bb, keys, plane_cells); break;
            case 4: launch_tile<4>(e, gd, b, bb, keys, plane_cells); break;
            case 5: launch_tile<5>(e, gd, b, bb, keys, plane_cells); break;
            case 6: launch_tile<6>(e, gd, b, bb, keys, plane_cells); break;
            case 7: launch_tile<7>(e, gd, b, bb, keys, plane_cells); break;
            default: launch_tile<8>(e, gd, b, bb, keys, plane_cells); break;
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

int pcr_hip_extremes_band(const pcr_hip_grid* g, const uint32_t* d_keys, int k, int side, float max_gap, float* d_out,
                          float* d_values, pcr_hip_stream s) {
    if (int rc = check_band_args(g, d_keys, k, side, max_gap, d_out)) return rc;
    const int own_rows = g->own_row1 - g->own_row0;
    if (own_rows <= 0) return PCR_HIP_OK;
    const int64_t cells = (int64_t)own_rows * g->width;
    const unsigned blocks = (unsigned)((cells + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(k_ext_band, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(s), g->width, own_rows,
                       g->own_row0 - g->state_row0, d_keys, (int64_t)g->state_rows * g->width, k, side, max_gap, d_out, d_values);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_extremes_band_host(const pcr_hip_grid* g, const uint32_t* h_keys, int k, int side, float max_gap, float* h_out,
                               float* h_values) {
    if (int rc = check_band_args(g, h_keys, k, side, max_gap, h_out)) return rc;
    const int own_rows = g->own_row1 - g->own_row0, W = g->width;
    const int64_t plane_cells = (int64_t)g->state_rows * W, cells = (int64_t)std::max(own_rows, 0) * W;
    const uint32_t* base = h_keys + (int64_t)(g->own_row0 - g->state_row0) * W;
    for (int64_t cell = 0; cell < cells; ++cell)
        h_out[cell] = ext::band_of(base + cell, plane_cells, k, side, max_gap, h_values ? h_values + cell : nullptr, cells);
    return PCR_HIP_OK;
}

}  // extern "C"
