// trees.h -- internal: segment_trees (pcr/core/trees.h) on the host, header-only so that a program can drive it without the rest
// of the library, and what the pipelines need of it.  The contract and the host twin are csrc/trees.hpp, the lines the HIP
// kernels compile.
#pragma once

#include "../../csrc/trees.hpp"
#include "pcr/core/grid.h"
#include "pcr/core/trees.h"
#include "pcr/core/types.h"
#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"
#include "terrain.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace pcr {
namespace detail {

namespace tt = pcrhip::trees;

/// "" when the spec is inside its ranges, else what is wrong with which field.
inline std::string tree_spec_error(const TreeSpec& s) {
    if (!std::isfinite(s.min_height)) return "min_height must be finite";
    if (!std::isfinite(s.window_base) || !(s.window_base >= 0.0f)) return "window_base must be finite and not negative";
    if (!std::isfinite(s.window_slope) || !(s.window_slope >= 0.0f)) return "window_slope must be finite and not negative";
    if (s.max_radius_cells < 1 || s.max_radius_cells > tt::kMaxRadius) return "max_radius_cells must be between 1 and 32";
    if (!std::isfinite(s.min_crown_height)) return "min_crown_height must be finite";
    if (!(s.crown_ratio >= 0.0f && s.crown_ratio <= 1.0f)) return "crown_ratio must be between 0 and 1";
    if (!(s.max_crown_radius > 0.0f)) return "max_crown_radius must be positive (+Inf: no limit)";
    return std::string();
}
inline bool tree_cell_sizes_ok(double cx, double cy) { return std::isfinite(cx) && cx != 0.0 && std::isfinite(cy) && cy != 0.0; }

/// The constants of a host loop, of a spec and cell sizes that passed the checks above.
inline tt::Consts tree_consts(const TreeSpec& s, double cell_size_x, double cell_size_y) {
    const double cell = std::max(std::fabs(cell_size_x), std::fabs(cell_size_y));
    tt::Consts k;
    k.min_height = s.min_height;
    k.window_base = s.window_base;
    k.window_slope = s.window_slope;
    k.max_radius = s.max_radius_cells;
    k.min_crown_height = s.min_crown_height;
    k.crown_ratio = s.crown_ratio;
    k.k = tt::k_of(cell);
    k.M = tt::M_of(s.max_crown_radius, cell);
    return k;
}
/// ... and what the C-ABI takes.
inline pcr_hip_tree_params tree_params(const TreeSpec& s, double cell_size_x, double cell_size_y) {
    pcr_hip_tree_params p{};
    p.min_height = s.min_height;
    p.window_base = s.window_base;
    p.window_slope = s.window_slope;
    p.max_radius_cells = s.max_radius_cells;
    p.min_crown_height = s.min_crown_height;
    p.crown_ratio = s.crown_ratio;
    p.max_crown_radius = s.max_crown_radius;
    p.cell_size_x = cell_size_x;
    p.cell_size_y = cell_size_y;
    return p;
}

/// The cell centres of a table's rows: by `geometry` when there is one, else with min_x = 0 and max_y = 0.
inline void tree_centres(TreeTable& t, const GridConfig* geometry, double cell_size_x, double cell_size_y) {
    const double x0 = geometry ? geometry->bounds.min_x : 0.0, y0 = geometry ? geometry->bounds.max_y : 0.0;
    const double cx = geometry ? geometry->cell_size_x : cell_size_x, cy = geometry ? geometry->cell_size_y : cell_size_y;
    t.x.resize(t.row.size());
    t.y.resize(t.row.size());
    for (size_t i = 0; i < t.row.size(); ++i) {
        t.x[i] = x0 + ((double)t.col[i] + 0.5) * cx;
        t.y[i] = y0 + ((double)t.row[i] + 0.5) * cy;
    }
}
inline Status tree_table_too_long(int64_t n) {
    return Status::error(StatusCode::OutOfRange, "trees: " + std::to_string(n) + " trees: ids above 2^24 are not exact in a Float32 band, "
                                                 "no table is made (segment the band in parts)");
}

// One band on the host: both bands and the table (without the centres), rows `stride` floats apart.
inline Status trees_host(const float* src, int w, int h, int64_t stride, const tt::Consts& k, float* id_dst, int64_t id_stride,
                         float* height_dst, int64_t height_stride, TreeTable* table) {
    tt::HostTable t;
    const int64_t n = tt::host(src, w, h, stride, k, id_dst, id_stride, height_dst, height_stride, table ? &t : nullptr);
    if (!table) return Status::success();
    *table = TreeTable();
    if (n > tt::kMaxExactId) return tree_table_too_long(n);
    table->row = std::move(t.row);
    table->col = std::move(t.col);
    table->height = std::move(t.height);
    table->crown_cells = std::move(t.crown_cells);
    return Status::success();
}

// The table a pcr_hip_trees enqueued on `stream` left in its work area (without the centres); waits for the stream (trees.cpp).
Status tree_table_device(const float* d_src, int w, int h, int64_t stride, const void* d_work, size_t work_bytes, void* stream,
                         TreeTable* out);

// ---- PipelineConfig::trees -------------------------------------------------------------------------------------------------
/// What a pipeline does about PipelineConfig::trees, decided at create.  The new bands follow the terrain bands, two per entry.
struct TreesPlan {
    struct Entry {
        int source = -1;                 // index of the source band in the result grid (an output, the DTM or the hag band)
        std::string id_name, height_name;
        TreeSpec spec;
    };
    std::vector<Entry> entries;
    double cell_size_x = 1.0, cell_size_y = -1.0;
    bool on() const { return !entries.empty(); }
    int extra_bands() const { return 2 * (int)entries.size(); }
};

inline Status plan_trees(const PipelineConfig& cfg, const GroundPlan& ground, const TerrainPlan& terrain, TreesPlan* plan) {
    *plan = TreesPlan();
    if (cfg.trees.empty()) return Status::success();
    auto refuse = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: " + msg); };
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0)
        return refuse("tree bands need the whole grid; derive them from the gathered grid with segment_trees");
    if (cfg.trees.size() > 4) return refuse("trees: more than 4 entries");
    std::vector<std::string> names = output_band_names(cfg);
    if (ground.on) {
        names.push_back(ground.dtm_name);
        if (ground.top >= 0) names.push_back(ground.hag_name);
    }
    const size_t n_sources = names.size();                // (terrain and tree bands are no sources)
    for (const auto& b : terrain.bands) names.push_back(b.name);
    if (!tree_cell_sizes_ok(cfg.grid.cell_size_x, cfg.grid.cell_size_y)) return refuse("tree bands need finite cell sizes that are not zero");
    plan->cell_size_x = cfg.grid.cell_size_x;
    plan->cell_size_y = cfg.grid.cell_size_y;
    for (size_t i = 0; i < cfg.trees.size(); ++i) {
        const TreeBandConfig& t = cfg.trees[i];
        const std::string where = "trees[" + std::to_string(i) + "]";
        TreesPlan::Entry e;
        const auto it = std::find(names.begin(), names.begin() + (std::ptrdiff_t)n_sources, t.source_band);
        if (t.source_band.empty() || it == names.begin() + (std::ptrdiff_t)n_sources)
            return refuse(where + ".source_band '" + t.source_band + "' names no source band of the result");
        e.source = (int)(it - names.begin());
        e.id_name = t.id_band_name.empty() ? t.source_band + "_tree_id" : t.id_band_name;
        e.height_name = t.height_band_name.empty() ? t.source_band + "_tree_height" : t.height_band_name;
        if (std::find(names.begin(), names.end(), e.id_name) != names.end())
            return refuse(where + ".id_band_name '" + e.id_name + "' clashes with another band");
        if (e.height_name == e.id_name || std::find(names.begin(), names.end(), e.height_name) != names.end())
            return refuse(where + ".height_band_name '" + e.height_name + "' clashes with another band");
        const std::string bad = tree_spec_error(t);
        if (!bad.empty()) return refuse(where + "." + bad);
        e.spec = t;
        names.push_back(e.id_name);
        names.push_back(e.height_name);
        plan->entries.push_back(e);
    }
    return Status::success();
}

/// The result grid's bands: ..., the terrain bands, then tree_id and tree_height of every entry in list order.
inline void append_tree_bands(const TreesPlan& plan, std::vector<BandDesc>& bands) {
    for (const auto& e : plan.entries) {
        BandDesc b;
        b.dtype = DataType::Float32;
        b.is_state = false;
        b.name = e.id_name;
        bands.push_back(b);
        b.name = e.height_name;
        bands.push_back(b);
    }
}

/// The tree bands of a host-resident result whose last plan.extra_bands() bands they are, from the source bands as they leave
/// the pipeline, and the tables (with centres by the result's geometry): behind the terrain bands.
inline Status trees_result_host(Grid& grid, const TreesPlan& plan, std::vector<TreeTable>* tables, std::vector<Status>* table_status) {
    if (tables) tables->assign(plan.entries.size(), TreeTable());
    if (table_status) table_status->assign(plan.entries.size(), Status::success());
    if (!plan.on()) return Status::success();
    const int w = grid.cols(), h = grid.rows();
    const int first = grid.num_bands() - plan.extra_bands();
    for (size_t i = 0; i < plan.entries.size(); ++i) {
        const auto& e = plan.entries[i];
        if (first < 0 || e.source >= first || !grid.band_f32(e.source))
            return Status::error(StatusCode::InvalidArgument, "pipeline: the result grid lacks the tree bands");
        TreeTable t;
        const Status s = trees_host(grid.band_f32(e.source), w, h, w, tree_consts(e.spec, plan.cell_size_x, plan.cell_size_y),
                                    grid.band_f32(first + 2 * (int)i), w, grid.band_f32(first + 2 * (int)i + 1), w, &t);
        tree_centres(t, grid.geometry(), plan.cell_size_x, plan.cell_size_y);
        if (tables) (*tables)[i] = std::move(t);
        if (table_status) (*table_status)[i] = s;           // (a table too long is the accessor's error, not finalize's)
    }
    return Status::success();
}

/// Everything behind the finalized bands of a host-resident result: finish_result_host with the terrain bands, then the tree bands.
inline Status finish_result_host(Grid& grid, std::vector<ReductionType> types, int fill_radius, const GroundPlan& ground,
                                 const TerrainPlan& terrain, const TreesPlan& trees, std::vector<TreeTable>* tables,
                                 std::vector<Status>* table_status) {
    Status s = finish_result_host(grid, std::move(types), fill_radius, ground, terrain, trees.extra_bands());
    return s.ok() ? trees_result_host(grid, trees, tables, table_status) : s;
}

}  // namespace detail
}  // namespace pcr
