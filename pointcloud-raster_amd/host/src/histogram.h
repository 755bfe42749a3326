// histogram.h -- (internal) what the pipelines share of PipelineConfig::histograms: the checks at create with one message
// each on every engine, the plan (bounds in binary64, band names, filter classes), and the percentile walk of the C-ABI's host
// twin shared out over OpenMP threads.  The arithmetic is csrc/histogram.hpp; the contract is in include/pcr_hip.h.
#pragma once

#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"
#include "pipeline_common.h"

#include <string>
#include <vector>

namespace pcr {
namespace detail {

constexpr size_t kMaxHistograms = 4;

/// One entry of PipelineConfig::histograms as the engines use it.
struct HistogramEntry {
    std::string value_channel;
    int bins = 0;
    double lo = 0.0, inv_w = 0.0, w = 0.0;       // inv_w = bins / (hi - lo), w = (hi - lo) / bins: computed here, once
    int cls = 0;                                 // its filter class (FilterPlan::hist_class_of)
    std::vector<float> q;                        // one percentile band per entry
    size_t cube_cells(size_t window_cells) const { return (size_t)bins * window_cells; }
};
struct HistogramPlan {
    std::vector<HistogramEntry> entries;
    int extra_bands() const {
        size_t n = 0;
        for (const auto& e : entries) n += e.q.size();
        return (int)n;
    }
};

/// create()'s refusals that do not depend on the engine (InvalidArgument): more than kMaxHistograms entries, bins outside
/// 1..256, non-finite bounds or lo >= hi, more than 16 percentiles, a percentile outside [0, 1] or NaN, an empty
/// value_channel, band_names longer than percentiles, a band name that collides with any other band that leaves the
/// pipeline, a row-block shard.  An empty list refuses nothing.
Status check_histograms(const PipelineConfig& cfg);
/// The refusals of ONE spec that PointZonalConfig::histograms shares, `where` naming the spec, in this order: value_channel, bins,
/// the bounds, more than 16 percentiles, a percentile outside [0, 1].
Status check_histogram_spec(const HistogramConfig& h, const std::string& where);
/// ... and the one of a pipeline that has to run out of core.
Status histograms_out_of_core_error();
/// ... and of the calls that would lose the cube (save_state, load_state, resume): NotImplemented.
Status histograms_checkpoint_error();
/// The plan of a configuration that passed check_histograms; `filters` is the configuration's plan_filters.
HistogramPlan plan_histograms(const PipelineConfig& cfg, const FilterPlan& filters);
/// One spec that passed its checks as an entry of filter class `cls`: the one place that computes lo, inv_w and w.
HistogramEntry histogram_entry(const HistogramConfig& h, int cls);
/// Bytes of every cube of the configuration over a window of `rows` rows: what counts towards gpu_memory_budget.
size_t histogram_cube_bytes(const PipelineConfig& cfg, size_t rows);

/// pcr_hip_histogram_percentiles_host over `threads` OpenMP threads, the rows shared out (every cell is independent).
/// counts: [bins][rows * width]; outs: e.q.size() bands of rows * width floats.
Status percentiles_host(const HistogramEntry& e, const uint32_t* counts, int width, int rows, float* const* outs, int threads);

}  // namespace detail
}  // namespace pcr
