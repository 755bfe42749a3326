// point_zonal.h -- (internal) what the pipelines and pcr::point_zonal share of PipelineConfig::point_zonal: the ONE plan routine with
// every refusal (one message each on every engine), the tables' memory, the fold of one ingest -- through the C-ABI's kernels on
// device memory, through its host twins on host memory -- and the one routine that makes a table.  A spec's refusals and its
// entry are cell_stats.h's and histogram.h's, the columns of a table zone_rows.h's: what the per-cell zonal tables (zonal.h) use
// too.  The arithmetic is csrc/point_zonal.hpp; the contract is in include/pcr_hip.h ("point zonal tables").
#pragma once

#include "../../csrc/point_zonal.hpp"
#include "buffer.h"
#include "cell_stats.h"
#include "histogram.h"
#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"
#include "pipeline_common.h"

#include <functional>
#include <string>
#include <vector>

namespace pcr {
namespace detail {

constexpr size_t kMaxPointZonal = 4;         // entries
constexpr size_t kMaxPointZonalSpecs = 4;    // stats specs, and histograms, per entry

/// PipelineConfig::point_zonal as the engines use it.
struct PointZonalPlan {
    struct Entry {
        std::string label;
        uint32_t Z = 0;                          // max_zones
        std::vector<CellStatsEntry> stats;       // cell_stats.h's and histogram.h's entries, from the same routines: `products`
        std::vector<HistogramEntry> hists;       // is not read, `cls` is FilterPlan::pz_stat_class_of / pz_hist_class_of
        // The entry's state, 64-bit words: [info 0, info 1][points Z][per stats spec: n Z, s1 Z, s2 Z][per histogram: counts Z * bins]
        size_t words() const;
        size_t points_at() const { return 2; }
        size_t stat_at(size_t k) const { return 2 + (size_t)Z * (1 + 3 * k); }
        size_t hist_at(size_t k) const;
    };
    std::vector<Entry> entries;
    bool on() const { return !entries.empty(); }
};

/// create()'s refusals (InvalidArgument) and, when it passes, the plan.  An empty list refuses nothing.
Status plan_point_zonal(const PipelineConfig& cfg, const FilterPlan& filters, PointZonalPlan* plan);
/// Bytes of every entry's state: max_zones * (8 + 24 * stats + 8 * sum of bins) + the info words; counts towards gpu_memory_budget.
size_t point_zonal_state_bytes(const PipelineConfig& cfg);
/// ... the refusal of a pipeline that has to run out of core, and of the calls that would lose the tables (NotImplemented).
Status point_zonal_out_of_core_error();
Status point_zonal_checkpoint_error();
/// What an ingest checks of a cloud before any state changes: every entry's label and value channels (derived ones apart) and its
/// specs' filters' channels.
Status validate_point_zonal(const PipelineConfig& cfg, const PointCloud& cloud);

/// The tables, entry by entry, zeroed: in `loc` memory (on `stream`, which is not waited for).
struct PointZonalState {
    std::vector<Buffer> tables;
    Status allocate(const PointZonalPlan& plan, MemoryLocation loc, void* stream);
};

/// One ingest's points: `channel` answers pointers into device (or host) memory, `mask(cls)` the byte mask of a filter class --
/// PipelineConfig::filter AND the class's own -- or null where every point is kept.
struct PointZonalInputs {
    bool device = false;
    void* stream = nullptr;
    size_t n = 0;
    ChannelLookup channel;
    std::function<const uint8_t*(int cls)> mask;
};
/// Every entry's folds for these points; on the device they are enqueued on in.stream, nothing is waited for.  `points` and the
/// info words take PipelineConfig::filter's survivors (class 0).
Status point_zonal_fold(const PointZonalPlan& plan, PointZonalState& state, const PointZonalInputs& in);

/// Entry e's table.  On the device everything is enqueued on `stream`, which is waited for twice: for the info words and for the
/// table.
Status point_zonal_table(const PointZonalPlan::Entry& e, const Buffer& table, void* stream, bool with_counts, PointZonalTable* out);

}  // namespace detail
}  // namespace pcr
