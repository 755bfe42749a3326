// histogram.cpp -- see histogram.h.
#include "histogram.h"

#include "buffer.h"

#include <algorithm>
#include <cmath>

namespace pcr {
namespace detail {

Status check_histogram_spec(const HistogramConfig& h, const std::string& where) {
    if (h.value_channel.empty()) return refuse(where + ".value_channel is empty");
    if (h.bins < 1 || h.bins > PCR_HIP_HISTOGRAM_MAX_BINS) return refuse(where + ".bins must be between 1 and 256");
    if (!std::isfinite(h.lo) || !std::isfinite(h.hi) || !(h.lo < h.hi)) return refuse(where + " needs finite bounds with lo < hi");
    if (h.percentiles.size() > PCR_HIP_HISTOGRAM_MAX_PERCENTILES) return refuse(where + " has more than 16 percentiles");
    for (float q : h.percentiles)
        if (!(q >= 0.0f && q <= 1.0f)) return refuse(where + ".percentiles must lie in [0, 1]");
    return Status::success();
}

Status check_histograms(const PipelineConfig& cfg) {
    const auto& list = cfg.histograms;
    if (list.empty()) return Status::success();
    if (list.size() > kMaxHistograms)
        return refuse("more than " + std::to_string(kMaxHistograms) + " histograms (" + std::to_string(list.size()) + " given)");
    for (size_t i = 0; i < list.size(); ++i) {
        const HistogramConfig& h = list[i];
        const std::string where = "histograms[" + std::to_string(i) + "]";
        if (Status s = check_histogram_spec(h, where); !s.ok()) return s;
        if (h.band_names.size() > h.percentiles.size()) return refuse(where + ".band_names is longer than percentiles");
    }
    // every band that leaves the pipeline, by name: the outputs (the percentile bands among them), the DTM and hag bands, the
    // terrain bands -- a percentile band's name may stand there once
    std::vector<std::string> names = output_band_names(cfg);
    if (!cfg.ground.source_band.empty()) {
        names.push_back(cfg.ground.dtm_band_name);
        if (!cfg.ground.top_band.empty()) names.push_back(cfg.ground.hag_band_name);
    }
    for (const auto& t : cfg.terrain)
        names.push_back(t.band_name.empty() ? t.source_band + "_" + terrain_product_name(t.product) : t.band_name);
    for (size_t i = 0; i < list.size(); ++i)
        for (size_t j = 0; j < list[i].percentiles.size(); ++j) {
            const std::string name = histogram_band_name(list[i], j);
            if (name.empty() || std::count(names.begin(), names.end(), name) != 1)
                return refuse("histograms[" + std::to_string(i) + "] band name '" + name + "' collides with another band");
        }
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0) return refuse("histograms are not supported on a row-block shard");
    return Status::success();
}

Status histograms_out_of_core_error() { return refuse("histograms are not supported on a pipeline that runs out of core"); }

Status histograms_checkpoint_error() {
    return Status::error(StatusCode::NotImplemented,
                         "pipeline: checkpoints do not carry the histograms' cubes yet: save_state, load_state and resume are "
                         "refused while PipelineConfig::histograms is not empty");
}

HistogramEntry histogram_entry(const HistogramConfig& h, int cls) {
    HistogramEntry e;
    e.value_channel = h.value_channel;
    e.bins = h.bins;
    e.lo = (double)h.lo;
    e.inv_w = (double)h.bins / ((double)h.hi - (double)h.lo);
    e.w = ((double)h.hi - (double)h.lo) / h.bins;
    e.cls = cls;
    e.q = h.percentiles;
    return e;
}

HistogramPlan plan_histograms(const PipelineConfig& cfg, const FilterPlan& filters) {
    HistogramPlan plan;
    for (size_t i = 0; i < cfg.histograms.size(); ++i)
        plan.entries.push_back(histogram_entry(cfg.histograms[i], i < filters.hist_class_of.size() ? filters.hist_class_of[i] : 0));
    return plan;
}

size_t histogram_cube_bytes(const PipelineConfig& cfg, size_t rows) {
    size_t bytes = 0;
    for (const auto& h : cfg.histograms) bytes += (size_t)std::max(h.bins, 0) * rows * (size_t)std::max(cfg.grid.width, 0) * sizeof(uint32_t);
    return bytes;
}

Status percentiles_host(const HistogramEntry& e, const uint32_t* counts, int width, int rows, float* const* outs, int threads) {
    if (e.q.empty() || rows <= 0 || width <= 0) return Status::success();
    const int chunk = 16;                                  // rows per call of the twin
    const int chunks = (rows + chunk - 1) / chunk;
    int failed = 0;
#pragma omp parallel for num_threads(std::max(threads, 1)) schedule(dynamic, 1)
    for (int c = 0; c < chunks; ++c) {
        // the twin on the rows [r0, r1) of the same window: the grid's owned rows narrowed, the bands' pointers moved along
        pcr_hip_grid g{};
        g.min_x = 0.0; g.min_y = 0.0; g.max_x = (double)width; g.max_y = (double)rows;
        g.cell_size_x = 1.0; g.cell_size_y = -1.0;
        g.width = width; g.height = rows;
        g.tile_width = width; g.tile_height = rows;
        g.state_row0 = 0; g.state_rows = rows;
        g.own_row0 = c * chunk; g.own_row1 = std::min(rows, g.own_row0 + chunk);
        float* moved[PCR_HIP_HISTOGRAM_MAX_PERCENTILES];
        for (size_t j = 0; j < e.q.size(); ++j) moved[j] = outs[j] + (size_t)g.own_row0 * width;
        if (pcr_hip_histogram_percentiles_host(&g, counts, e.bins, e.lo, e.w, (int)e.q.size(), e.q.data(), moved) != PCR_HIP_OK) {
#pragma omp atomic write
            failed = 1;
        }
    }
    return failed ? hip_status(PCR_HIP_INVALID_ARGUMENT) : Status::success();
}

}  // namespace detail
}  // namespace pcr
