// cell_stats.h -- (internal) what the pipelines share of PipelineConfig::cell_stats: the checks at create with one message each
// on every engine, the plan (filter classes, the reciprocal of the step), and the bands of the C-ABI's host twin shared out
// over OpenMP threads.  The arithmetic is csrc/cell_stats.hpp; the contract is in include/pcr_hip.h ("per-cell stats").
#pragma once

#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"
#include "pipeline_common.h"

#include <string>
#include <vector>

namespace pcr {
namespace detail {

constexpr size_t kMaxCellStats = 4;

/// One entry of PipelineConfig::cell_stats as the engines use it.
struct CellStatsEntry {
    std::string value_channel;
    double origin = 0.0, resolution = 0.0, inv_res = 0.0;    // inv_res = 1.0 / resolution: computed here, once
    int ddof = 0;
    int cls = 0;                                 // its filter class (FilterPlan::stat_class_of)
    std::vector<int> products;                   // PCR_HIP_CELL_STAT_*: one band per entry, in this order
};
struct CellStatsPlan {
    std::vector<CellStatsEntry> entries;
    int extra_bands() const {
        size_t n = 0;
        for (const auto& e : entries) n += e.products.size();
        return (int)n;
    }
};

/// create()'s refusals that do not depend on the engine (InvalidArgument): more than kMaxCellStats entries, an empty
/// value_channel, a resolution that is not finite and positive (or whose reciprocal is not finite), a non-finite origin, products
/// empty, longer than 3 or with a duplicate, ddof other than 0 or 1, band_names longer than products, a band name that collides
/// with any other band that leaves the pipeline, a row-block shard.  An empty list refuses nothing.
Status check_cell_stats(const PipelineConfig& cfg);
/// The refusals of ONE spec that PointZonalConfig::cell_stats shares, `where` naming the spec: value_channel, resolution and origin
/// -- and ddof, which check_cell_stats asks after the products.
Status check_cell_stats_value(const CellStatsConfig& c, const std::string& where);
Status check_cell_stats_ddof(const CellStatsConfig& c, const std::string& where);
/// ... and the one of a pipeline that has to run out of core.
Status cell_stats_out_of_core_error();
/// ... and of the calls that would lose the planes (save_state, load_state, resume): NotImplemented.
Status cell_stats_checkpoint_error();
/// The plan of a configuration that passed check_cell_stats; `filters` is the configuration's plan_filters.
CellStatsPlan plan_cell_stats(const PipelineConfig& cfg, const FilterPlan& filters);
/// One spec that passed its checks as an entry of filter class `cls`: the one place that computes inv_res.
CellStatsEntry cell_stats_entry(const CellStatsConfig& c, int cls);

/// pcr_hip_cell_stats_bands_host over `threads` OpenMP threads, the rows shared out (every cell is independent).
/// n, s1, s2: rows * width each; outs: one band of rows * width floats per product of the entry.
Status cell_stats_bands_host(const CellStatsEntry& e, const uint32_t* n, const int64_t* s1, const uint64_t* s2, int width, int rows,
                             float* const* outs, int threads);

}  // namespace detail
}  // namespace pcr
