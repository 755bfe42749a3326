// extremes.cpp -- see extremes.h.
#include "extremes.h"

#include "buffer.h"

#include <algorithm>
#include <cmath>

namespace pcr {
namespace detail {

Status check_extremes(const PipelineConfig& cfg) {
    const auto& list = cfg.extremes;
    if (list.empty()) return Status::success();
    if (list.size() > kMaxExtremes)
        return refuse("more than " + std::to_string(kMaxExtremes) + " extremes entries (" + std::to_string(list.size()) + " given)");
    for (size_t i = 0; i < list.size(); ++i) {
        const ExtremesConfig& e = list[i];
        const std::string where = "extremes[" + std::to_string(i) + "]";
        if (e.value_channel.empty()) return refuse(where + ".value_channel is empty");
        if (e.side != ExtremeSide::Lowest && e.side != ExtremeSide::Highest) return refuse(where + ".side is neither Lowest nor Highest");
        if (e.k < PCR_HIP_EXTREMES_MIN_K || e.k > PCR_HIP_EXTREMES_MAX_K) return refuse(where + ".k must be between 2 and 8");
        if (!(e.max_gap >= 0.0f)) return refuse(where + ".max_gap must not be negative or NaN");
    }
    // every band that leaves the pipeline, by name: the outputs (the extremes' bands among them), the DTM and hag bands, the
    // terrain bands -- an extremes band's name may stand there once
    std::vector<std::string> names = output_band_names(cfg);
    if (!cfg.ground.source_band.empty()) {
        names.push_back(cfg.ground.dtm_band_name);
        if (!cfg.ground.top_band.empty()) names.push_back(cfg.ground.hag_band_name);
    }
    for (const auto& t : cfg.terrain)
        names.push_back(t.band_name.empty() ? t.source_band + "_" + terrain_product_name(t.product) : t.band_name);
    for (size_t i = 0; i < list.size(); ++i) {
        const std::string name = extremes_band_name(list[i]);
        if (name.empty() || std::count(names.begin(), names.end(), name) != 1)
            return refuse("extremes[" + std::to_string(i) + "] band name '" + name + "' collides with another band");
    }
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0) return refuse("extremes are not supported on a row-block shard");
    return Status::success();
}

Status extremes_out_of_core_error() { return refuse("extremes are not supported on a pipeline that runs out of core"); }

Status extremes_checkpoint_error() {
    return Status::error(StatusCode::NotImplemented,
                         "pipeline: checkpoints do not carry the extremes' key planes yet: save_state, load_state and resume are "
                         "refused while PipelineConfig::extremes is not empty");
}

ExtremesPlan plan_extremes(const PipelineConfig& cfg, const FilterPlan& filters) {
    ExtremesPlan plan;
    for (size_t i = 0; i < cfg.extremes.size(); ++i) {
        const ExtremesConfig& c = cfg.extremes[i];
        ExtremesEntry e;
        e.value_channel = c.value_channel;
        e.k = c.k;
        e.side = c.side == ExtremeSide::Highest ? PCR_HIP_EXTREMES_HIGHEST : PCR_HIP_EXTREMES_LOWEST;
        e.max_gap = c.max_gap;
        e.cls = i < filters.ext_class_of.size() ? filters.ext_class_of[i] : 0;
        plan.entries.push_back(e);
    }
    return plan;
}

size_t extremes_state_bytes(const PipelineConfig& cfg, size_t rows) {
    size_t bytes = 0;
    for (const auto& e : cfg.extremes) bytes += (size_t)std::max(e.k, 0) * rows * (size_t)std::max(cfg.grid.width, 0) * sizeof(uint32_t);
    return bytes;
}

Status extremes_band_host(const ExtremesEntry& e, const uint32_t* keys, int width, int rows, float* out, float* values, int threads) {
    if (rows <= 0 || width <= 0) return Status::success();
    // the twin on the rows [r0, r1) of the same window: the grid's owned rows narrowed, the band's pointer moved along.  The
    // decoded planes lie one whole window apart, which the twin takes from its owned rows: asked for, the walk is one call.
    const int chunk = values ? rows : 16;
    const int chunks = (rows + chunk - 1) / chunk;
    int failed = 0;
#pragma omp parallel for num_threads(std::max(threads, 1)) schedule(dynamic, 1)
    for (int c = 0; c < chunks; ++c) {
        pcr_hip_grid g{};
        g.min_x = 0.0; g.min_y = 0.0; g.max_x = (double)width; g.max_y = (double)rows;
        g.cell_size_x = 1.0; g.cell_size_y = -1.0;
        g.width = width; g.height = rows;
        g.tile_width = width; g.tile_height = rows;
        g.state_row0 = 0; g.state_rows = rows;
        g.own_row0 = c * chunk; g.own_row1 = std::min(rows, g.own_row0 + chunk);
        if (pcr_hip_extremes_band_host(&g, keys, e.k, e.side, e.max_gap, out + (size_t)g.own_row0 * width, values) != PCR_HIP_OK) {
#pragma omp atomic write
            failed = 1;
        }
    }
    return failed ? hip_status(PCR_HIP_INVALID_ARGUMENT) : Status::success();
}

}  // namespace detail
}  // namespace pcr
