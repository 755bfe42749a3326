// engine.hpp -- the scatter engine object behind pcr_hip_engine_* / pcr_hip_scatter_*.
#pragma once

#include "common.hpp"

#include <functional>
#include <map>
#include <vector>

struct pcr_hip_engine {
    pcr_hip_grid grid{};
    pcrhip::GridDev gd{};
    hipStream_t stream = nullptr;
    int device = 0;
    int num_cus = 256;
    size_t lds_limit = 64 * 1024;              // LDS one workgroup may have on this device (queried at create)

    uint32_t* d_touched = nullptr;             // tiles_x * tiles_y words
    int ntiles = 0;
    unsigned long long* d_counters = nullptr;  // [0] = valid points of the scatter in flight; [8..16): what the last binned
                                               // Point / MostRecent scatter published (see counters_published)

    // Bin counts of the binning passes (bin_points): [kVirtualXcds][kMaxBins] for the first level, then [kMaxTiles] for the
    // second.  Owned by the engine (not carved from the shared scratch) because of their invariant: ALL ZERO whenever no
    // scatter of this engine is in flight -- zeroed once at create, and k_bin_scan, their last reader, writes the zeros back
    // as it goes.  So no launch has to run ahead of the count pass.  (913 KB whatever the grid: the tile shape, and with it
    // the number of bins, depends on the glyph and the planes of each scatter.)
    unsigned* d_bin_counts = nullptr;
    bool counts_clean = false;                 // cleared before a count pass is enqueued, set once the last scan of that
                                               // bin_points is: a scatter that finds it cleared (an earlier one failed half
                                               // way) zeroes the arrays itself
    // The same for d_counters[0..8) on the binned Point / MostRecent paths (publish_counters set by their entry points): the
    // first k_bin_scan of a scatter moves the eight words to [8..16) (further scans -- row bands -- add to them) and zeroes
    // the live ones.  Every other path zeroes them at its start and leaves them as they end up (engine.hip: zero_counters).
    bool counters_clean = false;               // [0..8) are zero once the stream reaches the next scatter
    bool publish_counters = false;             // the scatter being enqueued publishes through its scans
    bool counters_published = false;           // pcr_hip_engine_stats reads [8..16) (else [0..8))

    int forced_path = 0;                       // 0 auto, 1 direct, 2 binned, 3 moments (Gaussian only)
    int max_bins = 0;                          // LDS tiles per binning pass (kMaxBins; PCR_HIP_DEBUG_MAX_BINS lowers it
                                               // so that tests reach the large-grid paths on small grids)
    int stats_scatter_chunk = 0;               // points per k_bin_scatter workgroup of the last binned scatter
    bool two_level = true;                     // PCR_HIP_DEBUG_TWO_LEVEL=0 forces the row-band sweep instead
    pcr_hip_scatter_stats stats{};
    int planes_fresh = 0;                      // pcr_hip_engine_planes_fresh, for the NEXT scatter: 0 its planes hold earlier
                                               // contributions, 1 they hold identity values, 2 they are UNDEFINED (the
                                               // scatter defines every cell of the state window, see engine.hip)

    // pcr_hip_engine_finalize_with_scatter, for the NEXT Point scatter: bands its tile pass may store (scatter_binned.hip)
    pcrhip::FinalizeOuts fused_outs{};
    uint32_t* fused_done = nullptr;
    bool fused_taken = false;
    // pcr_hip_engine_defer_planes, for the same scatter: planes it may leave in those bands, and the ones it did
    uint32_t defer_planes = 0;
    uint32_t deferred_taken = 0;

    // optional per-kernel event timing
    bool profiling = false;
    std::string profile_only;                  // non-empty: only launches timed under this name are bracketed by events
    struct Pending { const char* name; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::map<std::string, std::pair<uint32_t, double>> kernel_ms;

    // pcr_hip_scatter_histogram, binned path (histogram.hip): the points' bin words, grow-only, the engine's own (the scratch
    // arena is carved anew by every pass of a sweep), and S, the bin planes an LDS tile holds (PCR_HIP_DEBUG_HIST_SLAB: 8, 16
    // or 32, for the measurement that chose the default).  pcr_hip_scatter_extremes (extremes.hip) keeps its key words in the
    // same buffer: one scatter is in the making at a time, and the stream orders their uses.
    uint32_t* d_hist_words = nullptr;
    size_t hist_words_cap = 0;                 // words
    int hist_slab = 16;                        // chosen by measurement: profiles/histogram.md

    // scratch of the binned / moment paths: borrowed per scatter from the device-wide arena (engine.hip)
    char* d_scratch = nullptr;
    size_t scratch_cap = 0;
    bool scratch_borrowed = false;
};

namespace pcrhip {

int ensure_scratch(pcr_hip_engine* e, size_t bytes);
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to the (device, kernel) pair and only ever has to grow: asked of the
// runtime when a launch needs more than any launch before it did, not on every launch (engine.hip).
void allow_dynamic_lds(const pcr_hip_engine* e, const void* kernel, size_t bytes);
// d_counters[0..8) = 0 on the engine's stream, for a path whose kernels count into them and leave them so (engine.hip).
int zero_counters(pcr_hip_engine* e);
void release_scratch(pcr_hip_engine* e);
// Device-resident tap tables of the moment path, shared by the engines of a device (engine.hip); call with the scratch
// borrowed.  fill(tables, K, r, sx, sy) builds the host copy when the glyph spec changed.
int shared_taps(pcr_hip_engine* e, int K, int r, float sx, float sy,
                void (*fill)(std::vector<float>&, int, int, float, float), const float** d_taps, size_t* count);

// Brackets one kernel launch with events when profiling is on.
struct ScopedKernelTimer {
    pcr_hip_engine* e;
    const char* name;
    hipEvent_t a = nullptr, b = nullptr;
    ScopedKernelTimer(pcr_hip_engine* eng, const char* nm) : e(eng), name(nm) {
        if (!e->profiling) return;
        if (!e->profile_only.empty() && e->profile_only != nm) return;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { a = b = nullptr; return; }
        (void)hipEventRecord(a, e->stream);
    }
    ~ScopedKernelTimer() {
        if (!a) return;
        (void)hipEventRecord(b, e->stream);
        e->pending.push_back({name, a, b});
    }
};

// ---- binning (counting sort of points by LDS tile), scatter_binned.hip ------------------------
struct BinGeom {
    int tile_w, tile_h;                 // interior of an LDS tile, cells (a bin owns these cells)
    int bins_x, bins_y, nbins;
    int chunk;                          // points per workgroup in the count / scatter passes: set by the front end that
                                        // picks the scatter shape (bin_points; the callers of b16::bin, bin16.hpp)
    int row0, rows;                     // the band of state rows [row0, row0 + rows) the bins cover (window-relative)
    int sup_shift;                      // two-level sort: the first level groups 2^sup_shift consecutive tiles (0: one level)
};
constexpr int kMaxBands = 32;           // a grid with more LDS tiles than kMaxBins is swept in row bands
struct BinItem {                        // one workgroup's share of a bin's records
    unsigned bin, first, count, shared; // shared != 0: the bin was split, merge with atomics
};
// Undefined planes whose tile pass merges a split bin with atomics need their identity values after all (n_items[1], known
// once the scan has run).  The scatter pass takes the fill along: every k_bin_scatter workgroup, its records out, reads
// n_items[1] and, only if it is set, stores its grid-stride share -- the usual case costs one scalar load per workgroup
// where a launch of 2 048 no-op workgroups (k_fill_if) stood on the stream.
struct TailFill {
    const unsigned* n_items;            // set by bin_points; null: nothing to fill
    void* plane[4];                     // 16-byte aligned, n16 groups of 16 bytes each; null: skipped
    unsigned bits[4];                   // the 32-bit pattern of plane p
    long long n16;
};
struct BinBuffers {                     // device pointers into the engine's scratch arena
    const uint2* records;               // Value / Index records, grouped by bin; .x = local cell
    const BinItem* items;
    const unsigned* n_items;            // [0] = items, [1] = 1 when some bin was split into several items
    int max_items;
    void* extra;                        // extra_bytes of the same scratch allocation, 256-B aligned, for the caller's own pass
    bool fill_folded;                   // the TailFill given to bin_points went with the scatter pass (one sort level); else
                                        // the tile pass fills behind the last scan itself
};
constexpr int kVirtualXcds = 8;         // record sub-ranges per bin (bin_points)
constexpr int kMaxBins = 12160;        // scatter pass LDS: the 8192-record staging window (64 KB) + 8 B per bin = 159 KB of the CU's 160.
                                        // Round 5 (8064 until then, "beyond this a block's runs are single records anyway"): measured on
                                        // the window of a C5 shard at N = 2 (16384 x 8192, 11 008 tiles, 500 M points) one level with
                                        // runs of ~2 records costs 5.79 ms a step, the two-level sort 7.18, two row bands 9.09
                                        // (tools/n2_shard_ab.sh) -- the second level's two passes over the records cost more than the
                                        // partial lines do.  Beyond this: two-level sort / row bands.
constexpr int kLcellBits = 15;          // up to 32768 cells per LDS tile
constexpr int kMaxTiles = 1 << (32 - kLcellBits);   // routing key = tile << 15 | local cell
constexpr int kMaxSubBins = 2048;       // tiles per first-level group (second-level scatter: 128 KB staging + 12 B per tile)

// Rows per band so that a band's bins fit the binning passes (whole tile rows); 0 = cannot be banded.
inline int band_rows_for(const GridDev& g, int tile_w, int tile_h, int max_bins) {
    const int bins_x = (g.W + tile_w - 1) / tile_w;
    const int bins_y = max_bins / bins_x;
    if (bins_y < 1) return 0;
    const int64_t rows = (int64_t)bins_y * tile_h;
    return (int)(rows < g.st_rows ? rows : g.st_rows);
}

// The engine's grid with the owned rows narrowed to the band [row0, row0 + rows) of state rows (empty: own_r0 >= own_r1).
inline GridDev band_grid(const GridDev& g, int row0, int rows) {
    GridDev gd = g;
    gd.own_r0 = std::max(g.own_r0, g.st_r0 + row0);
    gd.own_r1 = std::min(g.own_r1, g.st_r0 + row0 + rows);
    return gd;
}
// What a binned scatter reports (pcr_hip_scatter_stats): path 1 LDS tiles, 2 moments.
inline void set_binned_stats(pcr_hip_engine* e, int path, int tile_w, int tile_h, int apron, int bins) {
    e->stats.path = path;
    e->stats.lds_tile_w = tile_w;
    e->stats.lds_tile_h = tile_h;
    e->stats.lds_apron = apron;
    e->stats.num_bins = bins;
}

// Passes A (histogram + routing keys), scan, B (LDS-staged scatter) over the points that gd owns (for a band:
// the engine's grid with the owned rows narrowed to the band).  b.sup_shift > 0: the two-level counting sort for windows with
// more tiles than one pass counts -- A, scan, B on groups of 2^sup_shift tiles, then every group by tile (k_sub_count, scan,
// k_sub_scatter); item_records and every_bin apply to the last level.  Record kinds:
//   Value  8 B {local cell, value}         Point glyph
//   Index  8 B {local cell, point index}   MostRecent; Gaussian tiles with per-point sigma / rotation channels or r > 3 (the
//                                          others, and Lines, bin 16-byte value records: bin16.hpp)
enum class RecordKind { Value, Index };
// every_bin: an item (possibly of zero records) for EVERY bin, so that the tile pass visits every cell of the band.
int bin_points(pcr_hip_engine* e, const GridDev& gd, const BinGeom& b, const double* x, const double* y, const float* v,
               uint64_t n, RecordKind kind, unsigned item_records, BinBuffers* out, bool every_bin = false,
               size_t extra_bytes = 0, const TailFill* fill = nullptr);
// Identity values (0, 0, -FLT_MAX, +FLT_MAX) into the planes of `mask` over the engine's state window (engine.hip).
int fill_identity(pcr_hip_engine* e, uint32_t mask, const PlanesDev& pl);

// One sweep over the tiles of the state window, `whole` being its bins (row0 = 0, rows = st_rows, sup_shift = 0): in one pass
// when bin_points can count them (one sort level, or two), else in up to kMaxBands row bands.  Every pass bins the points of
// its rows (8-byte records, bin_points' arguments) and calls tile_pass with the pass's grid, bins and buffers; a non-zero
// status from it ends the sweep.  Returns the bins visited, or minus the error code.
// sweep_passes: the passes the sweep would take; 1 = the whole window at once, 0 = it cannot be binned.
using TilePass = std::function<int(const GridDev& gd, const BinGeom& b, const BinBuffers& bb)>;
int sweep_passes(const pcr_hip_engine* e, const BinGeom& whole);
int sweep_tiles(pcr_hip_engine* e, const BinGeom& whole, const double* x, const double* y, const float* v, uint64_t n,
                RecordKind kind, unsigned item_records, bool every_bin, size_t extra_bytes, const TilePass& tile_pass,
                const TailFill* fill = nullptr);

// direct path (global atomics), scatter_direct.hip
int direct_point(pcr_hip_engine* e, uint32_t mask, const PlanesDev& pl,
                 const double* x, const double* y, const float* v, uint64_t n);
int direct_glyph(pcr_hip_engine* e, const GlyphDev& gl, uint32_t mask, const PlanesDev& pl,
                 const double* x, const double* y, const float* v, uint64_t n);

// binned path (LDS tiles), scatter_binned.hip
bool binned_point_supported(const pcr_hip_engine* e, uint32_t mask);
int binned_point(pcr_hip_engine* e, uint32_t mask, const PlanesDev& pl,
                 const double* x, const double* y, const float* v, uint64_t n);
bool binned_glyph_supported(const pcr_hip_engine* e, const GlyphDev& gl, uint32_t mask);
int binned_glyph(pcr_hip_engine* e, const GlyphDev& gl, uint32_t mask, const PlanesDev& pl,
                 const double* x, const double* y, const float* v, uint64_t n);

// MostRecent (pcr_hip_scatter_select): one plane of packed 64-bit words, common.hpp select_word.  direct: scatter_direct.hip;
// binned: Index records through the Point front end (sweep_tiles), tile pass in scatter_binned.hip.
int direct_select(pcr_hip_engine* e, unsigned long long* packed, const double* x, const double* y, const float* v,
                  const float* key, uint64_t n);
bool binned_select_supported(const pcr_hip_engine* e);
int binned_select(pcr_hip_engine* e, unsigned long long* packed, const double* x, const double* y, const float* v,
                  const float* key, uint64_t n);

// Per-cell histograms (pcr_hip_scatter_histogram): a cube count[bins][state window] of uint32, histogram.hip.  direct: one
// global atomic add per accepted point; binned: VALUE records {local cell, bin} through the Point front end (sweep_tiles).
int direct_hist(pcr_hip_engine* e, uint32_t* counts, int bins, double lo, double inv_w, const double* x, const double* y,
                const float* v, uint64_t n);
bool binned_hist_supported(const pcr_hip_engine* e);
int binned_hist(pcr_hip_engine* e, uint32_t* counts, int bins, double lo, double inv_w, const double* x, const double* y,
                const float* v, uint64_t n);

// Per-cell extremes (pcr_hip_scatter_extremes): k planes keys[k][state window] of uint32, extremes.hip.  direct: the
// displacement chain with returning global atomics; binned: VALUE records {local cell, key} through the Point front end
// (sweep_tiles), the key words in d_hist_words.
int direct_extremes(pcr_hip_engine* e, uint32_t* keys, int k, int side, const double* x, const double* y, const float* v, uint64_t n);
bool binned_extremes_supported(const pcr_hip_engine* e, int k);
int binned_extremes(pcr_hip_engine* e, uint32_t* keys, int k, int side, const double* x, const double* y, const float* v, uint64_t n);

// Per-cell stats (pcr_hip_scatter_cell_stats): three integer planes N, S1, S2 over the state window, cell_stats.hip.  direct:
// three no-return global atomic adds per accepted point; binned: VALUE records {local cell, step} through the Point front end
// (sweep_tiles), the step words in d_hist_words (as the extremes' key words: one scatter is in the making at a time).
int direct_cell_stats(pcr_hip_engine* e, uint32_t* pn, long long* ps1, unsigned long long* ps2, double origin, double inv_res,
                      const double* x, const double* y, const float* v, uint64_t n);
bool binned_cell_stats_supported(const pcr_hip_engine* e);
int binned_cell_stats(pcr_hip_engine* e, uint32_t* pn, long long* ps1, unsigned long long* ps2, double origin, double inv_res,
                      const double* x, const double* y, const float* v, uint64_t n);

// Gaussian cell tiles on 16-byte value records (default-sigma, unrotated, r <= 3), scatter_cells.hip
bool cells_gauss_supported(const pcr_hip_engine* e, const GlyphDev& gl, uint32_t mask);
int cells_gauss(pcr_hip_engine* e, const GlyphDev& gl, uint32_t mask, const PlanesDev& pl,
                const double* x, const double* y, const float* v, uint64_t n);

// separable moment + convolution path for large default-sigma Gaussians, scatter_moments.hip
bool moments_supported(const pcr_hip_engine* e, const GlyphDev& gl, uint32_t mask);
// planes_undefined: the planes were only allocated (pcr_hip_engine_planes_fresh(e, 2)); the path defines every cell itself
int moments_gauss(pcr_hip_engine* e, const GlyphDev& gl, uint32_t mask, const PlanesDev& pl,
                  const double* x, const double* y, const float* v, uint64_t n, bool planes_undefined);

}  // namespace pcrhip
