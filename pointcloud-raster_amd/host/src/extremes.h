// extremes.h -- (internal) what the pipelines share of PipelineConfig::extremes: the checks at create with one message each on
// every engine, the plan (filter classes), and the band walk of the C-ABI's host twin shared out over OpenMP threads.  The
// arithmetic is csrc/extremes.hpp; the contract is in include/pcr_hip.h ("per-cell extremes").
#pragma once

#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"
#include "pipeline_common.h"

#include <string>
#include <vector>

namespace pcr {
namespace detail {

constexpr size_t kMaxExtremes = 4;

/// One entry of PipelineConfig::extremes as the engines use it.
struct ExtremesEntry {
    std::string value_channel;
    int k = 0;
    int side = PCR_HIP_EXTREMES_LOWEST;
    float max_gap = 0.0f;
    int cls = 0;                                 // its filter class (FilterPlan::ext_class_of)
    size_t state_cells(size_t window_cells) const { return (size_t)k * window_cells; }
};
struct ExtremesPlan {
    std::vector<ExtremesEntry> entries;
    int extra_bands() const { return (int)entries.size(); }
};

/// create()'s refusals that do not depend on the engine (InvalidArgument): more than kMaxExtremes entries, k outside 2..8, a
/// negative or NaN max_gap, an empty value_channel, an unknown side, a band name that collides with any other band that leaves
/// the pipeline, a row-block shard.  An empty list refuses nothing.
Status check_extremes(const PipelineConfig& cfg);
/// ... and the one of a pipeline that has to run out of core.
Status extremes_out_of_core_error();
/// ... and of the calls that would lose the key planes (save_state, load_state, resume): NotImplemented.
Status extremes_checkpoint_error();
/// The plan of a configuration that passed check_extremes; `filters` is the configuration's plan_filters.
ExtremesPlan plan_extremes(const PipelineConfig& cfg, const FilterPlan& filters);
/// Bytes of every entry's key planes over a window of `rows` rows: what counts towards gpu_memory_budget.
size_t extremes_state_bytes(const PipelineConfig& cfg, size_t rows);

/// pcr_hip_extremes_band_host over `threads` OpenMP threads, the rows shared out (every cell is independent).
/// keys: [k][rows * width]; out: rows * width floats; values: null or [k][rows * width] floats.
Status extremes_band_host(const ExtremesEntry& e, const uint32_t* keys, int width, int rows, float* out, float* values, int threads);

}  // namespace detail
}  // namespace pcr
