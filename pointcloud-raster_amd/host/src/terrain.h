// terrain.h -- internal: terrain (pcr/core/terrain.h) on the host, header-only so that a program can drive it without the rest
// of the library, and what the pipelines need of it.  The contract and the per-cell arithmetic are csrc/terrain.hpp, the lines
// the HIP kernel compiles.
#pragma once

#include "../../csrc/terrain.hpp"
#include "ground_filter.h"
#include "pcr/core/grid.h"
#include "pcr/core/terrain.h"
#include "pcr/core/types.h"
#include "pcr/engine/pipeline.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace pcr {
namespace detail {

namespace tr = pcrhip::terrain;

/// "" when the spec is inside its ranges, else what is wrong with which field.
inline std::string terrain_spec_error(const TerrainSpec& s) {
    if (!std::isfinite(s.z_factor) || s.z_factor == 0.0f) return "z_factor must be finite and not zero";
    if (!std::isfinite(s.azimuth)) return "azimuth must be finite";
    if (!(s.altitude >= 0.0f && s.altitude <= 90.0f)) return "altitude must be between 0 and 90";
    return std::string();
}
inline bool terrain_cell_sizes_ok(double cx, double cy) { return std::isfinite(cx) && cx != 0.0 && std::isfinite(cy) && cy != 0.0; }

/// The constants of a launch or a host loop, of a spec and cell sizes that passed the checks above.
inline tr::Consts terrain_consts(const TerrainSpec& s, double cell_size_x, double cell_size_y) {
    const TerrainLight l = terrain_light((double)s.azimuth, (double)s.altitude);
    tr::Consts k;
    k.kx = tr::scale((double)s.z_factor, 8.0, cell_size_x);
    k.ky = tr::scale((double)s.z_factor, -8.0, cell_size_y);
    k.sin_alt = l.sin_alt;
    k.ls = l.ls;
    k.lc = l.lc;
    return k;
}

// One band on the host: `n` distinct products (ids of csrc/terrain.hpp) of src into dsts, rows `src_stride` / `dst_strides[k]`
// floats apart, no dst overlapping src.  Rows are independent: the bits do not depend on how they are shared out.
inline void terrain_host(const float* src, int w, int h, int64_t src_stride, int n, const int* products, float* const* dsts,
                         const int64_t* dst_strides, const tr::Consts& k, int edges) {
    unsigned mask = 0;
    for (int i = 0; i < n; ++i) mask |= 1u << products[i];
    const float out = tr::nodata();
#pragma omp parallel for schedule(static) if ((int64_t)w * h > 4096)
    for (int r = 0; r < h; ++r) {
        const float* rows[3] = {r > 0 ? src + (int64_t)(r - 1) * src_stride : nullptr, src + (int64_t)r * src_stride,
                                r + 1 < h ? src + (int64_t)(r + 1) * src_stride : nullptr};
        for (int c = 0; c < w; ++c) {
            float w9[9];
            for (int d = 0; d < 3; ++d)
                for (int e = -1; e <= 1; ++e) {
                    float x = out;
                    if (rows[d] && c + e >= 0 && c + e < w) std::memcpy(&x, rows[d] + c + e, sizeof(float));
                    w9[3 * d + e + 1] = x;
                }
            float o[tr::kProducts] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            const bool ok = tr::window(w9, edges);
            tr::evaluate<true, true>(w9, ok, mask, k, o);
            for (int i = 0; i < n; ++i) std::memcpy(dsts[i] + (int64_t)r * dst_strides[i] + c, &o[products[i]], sizeof(float));
        }
    }
}

// ---- PipelineConfig::terrain -----------------------------------------------------------------------------------------------
/// What a pipeline does about PipelineConfig::terrain, decided at create.  The new bands follow the ground filter's in list order.
struct TerrainPlan {
    struct Band {
        int source = -1;                 // index of the source band in the result grid (an output, the DTM or the hag band)
        int product = 0;
        std::string name;
        TerrainSpec spec;
    };
    std::vector<Band> bands;
    // entries that share source, z_factor and compute_edges go into one launch: indices into `bands`, every product at most
    // once per launch (the light is the hillshade entry's: spec_of)
    std::vector<std::vector<int>> launches;
    const TerrainSpec& spec_of(const std::vector<int>& launch) const {
        for (int m : launch)
            if (bands[(size_t)m].product == tr::kHillshade) return bands[(size_t)m].spec;
        return bands[(size_t)launch.front()].spec;
    }
    double cell_size_x = 1.0, cell_size_y = -1.0;
    bool on() const { return !bands.empty(); }
    int extra_bands() const { return (int)bands.size(); }
};

inline Status plan_terrain(const PipelineConfig& cfg, const GroundPlan& ground, TerrainPlan* plan) {
    *plan = TerrainPlan();
    if (cfg.terrain.empty()) return Status::success();
    auto refuse = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: " + msg); };
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0)
        return refuse("terrain bands need the whole grid; derive them from the gathered grid with terrain");
    std::vector<std::string> names = output_band_names(cfg);
    if (ground.on) {
        names.push_back(ground.dtm_name);
        if (ground.top >= 0) names.push_back(ground.hag_name);
    }
    const size_t n_sources = names.size();
    if (!terrain_cell_sizes_ok(cfg.grid.cell_size_x, cfg.grid.cell_size_y)) return refuse("terrain bands need finite cell sizes that are not zero");
    plan->cell_size_x = cfg.grid.cell_size_x;
    plan->cell_size_y = cfg.grid.cell_size_y;
    for (size_t i = 0; i < cfg.terrain.size(); ++i) {
        const TerrainBandConfig& t = cfg.terrain[i];
        const std::string where = "terrain[" + std::to_string(i) + "]";
        TerrainPlan::Band b;
        const auto it = std::find(names.begin(), names.begin() + (std::ptrdiff_t)n_sources, t.source_band);
        if (t.source_band.empty() || it == names.begin() + (std::ptrdiff_t)n_sources)
            return refuse(where + ".source_band '" + t.source_band + "' names no band of the result");
        b.source = (int)(it - names.begin());
        const char* pname = terrain_product_name(t.product);
        if (!pname[0]) return refuse(where + ".product is no terrain product");
        b.product = (int)t.product;
        b.name = t.band_name.empty() ? t.source_band + "_" + pname : t.band_name;
        if (std::find(names.begin(), names.end(), b.name) != names.end())
            return refuse(where + ".band_name '" + b.name + "' clashes with another band");
        const std::string bad = terrain_spec_error(t);
        if (!bad.empty()) return refuse(where + "." + bad);
        b.spec = t;
        names.push_back(b.name);
        plan->bands.push_back(b);
    }
    for (size_t i = 0; i < plan->bands.size(); ++i) {
        const auto& b = plan->bands[i];
        bool placed = false;
        for (auto& l : plan->launches) {
            const auto& f = plan->bands[(size_t)l.front()];
            bool fits = f.source == b.source && f.spec.z_factor == b.spec.z_factor && f.spec.compute_edges == b.spec.compute_edges;
            for (int m : l) fits = fits && plan->bands[(size_t)m].product != b.product;
            if (fits) { l.push_back((int)i); placed = true; break; }
        }
        if (!placed) plan->launches.push_back({(int)i});
    }
    return Status::success();
}

/// The result grid's bands: ..., then the terrain bands in list order.
inline void append_terrain_bands(const TerrainPlan& plan, std::vector<BandDesc>& bands) {
    for (const auto& t : plan.bands) {
        BandDesc b;
        b.dtype = DataType::Float32;
        b.is_state = false;
        b.name = t.name;
        bands.push_back(b);
    }
}

/// The terrain bands of a host-resident result whose last plan.extra_bands() bands they are, from the source bands as they
/// leave the pipeline: after finish_result_host.
/// more_bands: bands that follow the terrain bands and are none of this function's business (trees.h).
inline Status terrain_result_host(Grid& grid, const TerrainPlan& plan, int more_bands = 0) {
    if (!plan.on()) return Status::success();
    const int w = grid.cols(), h = grid.rows();
    const int first = grid.num_bands() - plan.extra_bands() - more_bands;
    if (first < 0) return Status::error(StatusCode::InvalidArgument, "pipeline: the result grid lacks the terrain bands");
    for (const auto& l : plan.launches) {
        const auto& f = plan.bands[(size_t)l.front()];
        std::vector<int> products;
        std::vector<float*> dsts;
        std::vector<int64_t> strides;
        for (int m : l) {
            products.push_back(plan.bands[(size_t)m].product);
            dsts.push_back(grid.band_f32(first + m));
            strides.push_back(w);
        }
        if (f.source >= first || !grid.band_f32(f.source))
            return Status::error(StatusCode::InvalidArgument, "pipeline: the result grid lacks the terrain bands");
        terrain_host(grid.band_f32(f.source), w, h, w, (int)l.size(), products.data(), dsts.data(), strides.data(),
                     terrain_consts(plan.spec_of(l), plan.cell_size_x, plan.cell_size_y), f.spec.compute_edges ? 1 : 0);
    }
    return Status::success();
}

/// Everything behind the finalized bands of a host-resident result: finish_result_host, then the terrain bands.
inline Status finish_result_host(Grid& grid, std::vector<ReductionType> types, int fill_radius, const GroundPlan& ground,
                                 const TerrainPlan& terrain, int more_bands = 0) {
    if (terrain.on()) {
        // (finish_result_host counts the bands it was promised: it sees the grid without the terrain bands' share)
        const int first = grid.num_bands() - terrain.extra_bands() - more_bands;
        if (first != (int)types.size() + ground.extra_bands())
            return Status::error(StatusCode::InvalidArgument, "pipeline: the result grid lacks the terrain bands");
    }
    Status s = finish_result_host(grid, std::move(types), fill_radius, ground, terrain.extra_bands() + more_bands);
    return s.ok() ? terrain_result_host(grid, terrain, more_bands) : s;
}

/// The gathered grid of a sharded run on rank 0 (the reductions' bands, on the host) as the unsharded pipeline `whole_cfg`
/// would return it: the ground filter's and the terrain bands appended, then finish_result_host.
inline Status finish_gathered_host(std::unique_ptr<Grid>& whole, const PipelineConfig& whole_cfg) {
    GroundPlan ground;
    TerrainPlan terrain;
    Status s = plan_ground(whole_cfg, &ground);
    if (s.ok()) s = plan_terrain(whole_cfg, ground, &terrain);
    if (!s.ok()) return s;
    if (ground.on || terrain.on()) {
        std::vector<BandDesc> descs;
        for (int b = 0; b < whole->num_bands(); ++b) descs.push_back(whole->band_desc(b));
        append_ground_bands(ground, descs);
        append_terrain_bands(terrain, descs);
        std::unique_ptr<Grid> wider = Grid::create(whole->cols(), whole->rows(), descs, MemoryLocation::Host);
        if (!wider) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate the ground filter's and the terrain bands");
        for (int b = 0; b < whole->num_bands(); ++b)
            std::memcpy(wider->band_f32(b), whole->band_f32(b), (size_t)whole->cell_count() * sizeof(float));
        whole = std::move(wider);
    }
    std::vector<ReductionType> types;
    for (const auto& r : whole_cfg.reductions) types.push_back(r.type);
    return finish_result_host(*whole, types, whole_cfg.fill_nodata_radius, ground, terrain);
}

}  // namespace detail
}  // namespace pcr
