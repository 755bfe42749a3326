// host_pipeline.h -- (internal) Pipeline::Host: the pipeline on the host engine (host_engine.h), behind ExecutionMode::CPU,
// Auto without a GPU and gpu_fallback_to_cpu -- what the reference does in those cases (src/engine/pipeline.cpp:100-131).
// Same validation, messages, band naming, progress callback and `.pcrt` checkpoints as the HIP pipeline.
#pragma once

#include "histogram.h"
#include "host_engine.h"
#include "pcr/core/grid.h"
#include "pcr/engine/pipeline.h"
#include "pipeline_common.h"
#include "sample_grid.h"

#include <chrono>
#include <memory>
#include <string>
#include <vector>

namespace pcr {

struct Pipeline::Host {
    struct Group {                       // one pass over the points: same grouping as the HIP pipeline
        std::string value_channel;
        std::string key_channel;         // a MostRecent group: its timestamp channel
        bool select = false;
        GlyphSpec glyph;
        detail::HostPlanes planes;
        uint32_t mask = 0;
        FilterSpec filter;               // ReductionSpec::filter of the group's specs (part of the grouping key)
        int cls = 0;                     // its filter class (detail::FilterPlan): 0 = PipelineConfig::filter alone
    };
    struct Output {                      // one band finalize makes from the state: a ReductionSpec's, or a percentile band
        int group = 0;                   // -1: a percentile band of histogram `hist` (its type is Max: filled like a Max band)
        ReductionType type = ReductionType::Sum;
        std::string band_name;
        int hist = -1, q = 0;            // the histogram and which of its percentiles
    };

    PipelineConfig cfg;
    std::unique_ptr<detail::HostEngine> engine;
    std::vector<Group> groups;
    std::vector<Output> outputs;
    detail::FilterPlan filters;          // ReductionSpec::filter of every spec, planned at init
    std::vector<detail::Surface> surfaces;   // PipelineConfig::surface_channels, entry by entry: the band in host memory
    detail::HistogramPlan hist;          // PipelineConfig::histograms, planned at init
    std::vector<std::vector<uint32_t>> cubes;    // entry by entry: count[bins][height * width], zero at create
    std::unique_ptr<Grid> result;
    bool finalized = false;
    ProgressCallback callback;
    size_t collections = 0, points = 0;
    ScatterInfo last{};
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();

    Status init();
    Status ingest(const PointCloud& cloud);
    Status finalize();
    Status set_surface(const std::string& name, const Grid& grid, int band);
    Status save_state(const std::string& dir);
    Status load_state(const std::string& dir);
    ProgressInfo stats() const;
    std::vector<detail::StateOutput> state_outputs() const;
};

}  // namespace pcr
