// banded_pipeline.h -- (internal) Pipeline::Banded: the out-of-core driver.  A grid whose state exceeds the device budget is
// swept in row bands of whole reference-tile rows, one band in HBM at a time (a device pipeline created for the visit), the
// others parked in host memory and, beyond host_cache_budget, in `.pcrt` files -- the role of the reference's TileManager.
#pragma once

#include "pcr/core/grid.h"
#include "pcr/engine/pipeline.h"
#include "pipeline_common.h"

#include <chrono>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace pcr {

// ---- out-of-core grids: row bands of whole reference-tile rows ---------------------------------------------------
// The reference keeps every tile's state behind a TileManager: an LRU cache in memory, evicted tiles flushed to `.pcrt`
// files and loaded back on the next acquire (src/engine/tile_manager.cpp:76-138, 183-375), so that a grid may be larger
// than memory.  This build keeps the state of the WHOLE grid in HBM -- until it does not fit the budget.
// Then the grid is swept in bands of whole reference-tile rows: footprints are clipped to the reference tile of their
// centre cell (Q4), so nothing a band's points paint can land outside the band -- a band is an ordinary row-block shard
// with no halo to exchange.  One band's planes are in HBM at a time (a sub-pipeline created for the visit); the others are
// parked as host copies up to host_cache_budget and, least recently used first, in files under state_dir beyond it.  Every
// ingest visits every band (the kernels keep the points whose centre row the band owns); finalize visits them once more
// and assembles the host result.  Results are those of the in-core pipeline bit for bit: the same kernels run on the same
// points of each tile, in the same order.
struct Pipeline::Banded {
    PipelineConfig cfg;                                   // the WHOLE grid, as the caller gave it
    std::vector<std::pair<int, int>> bands;               // [r0, r1), multiples of the tile height
    detail::GroupPlan plan;                               // the groups and outputs of every band's sub-pipeline (parked planes[4 g + p])
    bool spec_filters = false;                            // some ReductionSpec has a filter of its own (detail::FilterPlan::any)
    struct Parked {
        bool any = false, on_disk = false;
        std::vector<std::vector<float>> planes;           // [4 g + p]: the band's window of plane p of group g (empty: no such plane)
        std::vector<uint32_t> touched;                    // tiles_x * tiles_y flags of the whole grid (only this band's rows are set)
        size_t bytes = 0;
        uint64_t stamp = 0;
        // the host copy goes (it is in the band's files): returns the bytes it held
        size_t release() {
            std::vector<std::vector<float>>().swap(planes);
            std::vector<uint32_t>().swap(touched);
            on_disk = true;
            return bytes;
        }
    };
    std::vector<Parked> parked;
    size_t host_budget = 0, host_used = 0, spills = 0, reloads = 0;
    uint64_t clock = 0;
    // Evicted bands live in the reference's own format and layout: one `.pcrt` file per touched reference tile and
    // ReductionSpec (tile_RRRR_CCCC.pcrt; reduction_<i>/ for several reductions) -- what the reference's TileManager flushes
    // on eviction (src/engine/tile_manager.cpp:76-138 -> src/io/tile_state_io.cpp:45-95) -- in a directory of the pipeline's
    // own (under state_dir, else the temporary directory), removed with the pipeline: a spill is working state, possibly
    // partial and older than a band's host copy, and must never be mistaken for a checkpoint.  save_state() writes one.
    std::string spill_dir;
    std::unique_ptr<Grid> result;
    bool finalized = false;
    std::vector<TreeTable> tree_tables;      // PipelineConfig::trees, entry by entry, as the last finalize left them
    std::vector<Status> tree_status;
    size_t collections = 0, points = 0, tiles_active = 0;
    ProgressCallback callback;
    ScatterInfo last{};
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();

    /// Out of core?  Only whole-grid pipelines (a row-block shard is somebody's band already), only when the state of the
    /// whole grid exceeds the device budget (*budget: gpu_memory_budget, or ~80 % of the free device memory).
    static bool needed(const PipelineConfig& config, size_t* budget);
    /// Plans the bands, sets up the spill directory (named after `owner`), creates the first band once -- so that an impossible
    /// configuration fails at create like an in-core one -- and resumes from state_dir when asked to.  nullptr + *st on failure.
    static std::unique_ptr<Banded> create(const PipelineConfig& config, const Pipeline* owner, size_t budget, Status* st);
    ~Banded();

    Status ingest(const PointCloud& cloud);
    Status finalize();
    Status save_state(const std::string& dir);
    Status load_state(const std::string& dir);
    ProgressInfo stats() const;

    static size_t bytes_per_row(const PipelineConfig& c);
    detail::StateWindow window_of(size_t b, Parked& k) const { return detail::window_over(k.planes, bands[b].first, bands[b].second - bands[b].first); }
    void blank(size_t b, Parked& k) const;
    Status spill(size_t b);
    Status reload(size_t b);
    void drop_host_copy(size_t b) { host_used -= parked[b].release(); }
    Status account(size_t b);
    Status evict();
    std::unique_ptr<Pipeline> visit(size_t b, Status* st, bool* was_on_disk = nullptr);
    Status count_kept(const PointCloud& dev, size_t* kept);
};

}  // namespace pcr
