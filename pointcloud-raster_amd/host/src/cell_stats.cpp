// cell_stats.cpp -- see cell_stats.h.
#include "cell_stats.h"

#include "buffer.h"

#include <algorithm>
#include <cmath>

namespace pcr {
namespace detail {

namespace {
bool known(CellStat p) { return p == CellStat::Mean || p == CellStat::Variance || p == CellStat::StdDev; }
}  // namespace

Status check_cell_stats_value(const CellStatsConfig& c, const std::string& where) {
    if (c.value_channel.empty()) return refuse(where + ".value_channel is empty");
    if (!std::isfinite(c.resolution) || !(c.resolution > 0.0) || !std::isfinite(1.0 / c.resolution))
        return refuse(where + ".resolution must be finite and positive");
    if (!std::isfinite(c.origin)) return refuse(where + ".origin must be finite");
    return Status::success();
}

Status check_cell_stats_ddof(const CellStatsConfig& c, const std::string& where) {
    if (c.ddof != 0 && c.ddof != 1) return refuse(where + ".ddof must be 0 or 1");
    return Status::success();
}

Status check_cell_stats(const PipelineConfig& cfg) {
    const auto& list = cfg.cell_stats;
    if (list.empty()) return Status::success();
    if (list.size() > kMaxCellStats)
        return refuse("more than " + std::to_string(kMaxCellStats) + " cell_stats entries (" + std::to_string(list.size()) + " given)");
    for (size_t i = 0; i < list.size(); ++i) {
        const CellStatsConfig& c = list[i];
        const std::string where = "cell_stats[" + std::to_string(i) + "]";
        if (Status s = check_cell_stats_value(c, where); !s.ok()) return s;
        if (c.products.empty() || c.products.size() > PCR_HIP_CELL_STATS_MAX_PRODUCTS)
            return refuse(where + ".products must name between 1 and 3 bands");
        for (size_t j = 0; j < c.products.size(); ++j) {
            if (!known(c.products[j])) return refuse(where + ".products names an unknown band");
            if (std::count(c.products.begin(), c.products.end(), c.products[j]) != 1) return refuse(where + ".products names a band twice");
        }
        if (Status s = check_cell_stats_ddof(c, where); !s.ok()) return s;
        if (c.band_names.size() > c.products.size()) return refuse(where + ".band_names is longer than products");
    }
    // every band that leaves the pipeline, by name: the outputs (the cell-stats bands among them), the DTM and hag bands, the
    // terrain bands -- a cell-stats band's name may stand there once
    std::vector<std::string> names = output_band_names(cfg);
    if (!cfg.ground.source_band.empty()) {
        names.push_back(cfg.ground.dtm_band_name);
        if (!cfg.ground.top_band.empty()) names.push_back(cfg.ground.hag_band_name);
    }
    for (const auto& t : cfg.terrain)
        names.push_back(t.band_name.empty() ? t.source_band + "_" + terrain_product_name(t.product) : t.band_name);
    for (size_t i = 0; i < list.size(); ++i)
        for (size_t j = 0; j < list[i].products.size(); ++j) {
            const std::string name = cell_stats_band_name(list[i], j);
            if (name.empty() || std::count(names.begin(), names.end(), name) != 1)
                return refuse("cell_stats[" + std::to_string(i) + "] band name '" + name + "' collides with another band");
        }
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0) return refuse("cell_stats are not supported on a row-block shard");
    return Status::success();
}

Status cell_stats_out_of_core_error() { return refuse("cell_stats are not supported on a pipeline that runs out of core"); }

Status cell_stats_checkpoint_error() {
    return Status::error(StatusCode::NotImplemented,
                         "pipeline: checkpoints do not carry the cell stats' planes yet: save_state, load_state and resume are "
                         "refused while PipelineConfig::cell_stats is not empty");
}

CellStatsEntry cell_stats_entry(const CellStatsConfig& c, int cls) {
    CellStatsEntry e;
    e.value_channel = c.value_channel;
    e.origin = c.origin;
    e.resolution = c.resolution;
    e.inv_res = 1.0 / c.resolution;
    e.ddof = c.ddof;
    e.cls = cls;
    for (CellStat p : c.products) e.products.push_back(static_cast<int>(p));
    return e;
}

CellStatsPlan plan_cell_stats(const PipelineConfig& cfg, const FilterPlan& filters) {
    CellStatsPlan plan;
    for (size_t i = 0; i < cfg.cell_stats.size(); ++i)
        plan.entries.push_back(cell_stats_entry(cfg.cell_stats[i], i < filters.stat_class_of.size() ? filters.stat_class_of[i] : 0));
    return plan;
}

Status cell_stats_bands_host(const CellStatsEntry& e, const uint32_t* n, const int64_t* s1, const uint64_t* s2, int width, int rows,
                             float* const* outs, int threads) {
    if (e.products.empty() || rows <= 0 || width <= 0) return Status::success();
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
        float* moved[PCR_HIP_CELL_STATS_MAX_PRODUCTS];
        for (size_t j = 0; j < e.products.size(); ++j) moved[j] = outs[j] + (size_t)g.own_row0 * width;
        if (pcr_hip_cell_stats_bands_host(&g, n, reinterpret_cast<const long long*>(s1), reinterpret_cast<const unsigned long long*>(s2),
                                          e.origin, e.resolution, e.ddof, (int)e.products.size(), e.products.data(), moved) != PCR_HIP_OK) {
#pragma omp atomic write
            failed = 1;
        }
    }
    return failed ? hip_status(PCR_HIP_INVALID_ARGUMENT) : Status::success();
}

}  // namespace detail
}  // namespace pcr
