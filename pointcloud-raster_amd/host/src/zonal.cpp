// zonal.cpp -- see zonal.h.
#include "zonal.h"

#include "pipeline_common.h"
#include "polygons.h"
#include "zone_rows.h"

#include <algorithm>
#include <cstring>

namespace pcr {
namespace detail {

namespace zn = pcrhip::zonal;

namespace {

const std::vector<float>& percentiles_of(const PipelineConfig& cfg, const ZonalConfig& z, int h) {
    return z.own_percentiles ? cfg.histograms[(size_t)h].percentiles : z.percentiles;
}

// The entry's columns as zone_rows.h names them: channels and percentiles, no table yet.
ZoneRowsInputs columns_of(const PipelineConfig& cfg, const ZonalConfig& z) {
    ZoneRowsInputs r;
    r.stats.resize(z.cell_stats.size());
    r.hists.resize(z.histograms.size());
    for (size_t k = 0; k < r.stats.size(); ++k) r.stats[k].channel = cfg.cell_stats[(size_t)z.cell_stats[k]].value_channel;
    for (size_t k = 0; k < r.hists.size(); ++k) {
        r.hists[k].channel = cfg.histograms[(size_t)z.histograms[k]].value_channel;
        r.hists[k].q = percentiles_of(cfg, z, z.histograms[k]);
    }
    return r;
}

}  // namespace

std::vector<std::string> zonal_column_names(const PipelineConfig& cfg, const ZonalConfig& z) {
    return zone_column_names("cells", columns_of(cfg, z));
}

Status zonal_out_of_core_error() {
    return refuse("zonal tables need the state in HBM: the grid does not fit gpu_memory_budget and would run out of core");
}

Status plan_zonal(const PipelineConfig& cfg, const GroundPlan& ground, const TerrainPlan& terrain, const TreesPlan& trees, ZonalPlan* plan) {
    *plan = ZonalPlan();
    if (cfg.zonal.empty()) return Status::success();
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0)
        return refuse("zonal tables need the whole grid: a row-block shard holds a part of every zone that crosses its edge");
    if (cfg.zonal.size() > kMaxZonal) return refuse("zonal: more than 4 entries");
    std::vector<std::string> names = output_band_names(cfg);
    if (ground.on) {
        names.push_back(ground.dtm_name);
        if (ground.top >= 0) names.push_back(ground.hag_name);
    }
    for (const auto& b : terrain.bands) names.push_back(b.name);
    for (const auto& t : trees.entries) {
        names.push_back(t.id_name);
        names.push_back(t.height_name);
    }
    for (size_t i = 0; i < cfg.zonal.size(); ++i) {
        const ZonalConfig& z = cfg.zonal[i];
        const std::string where = "zonal[" + std::to_string(i) + "]";
        ZonalPlan::Entry e;
        if (z.zones.empty()) return refuse(where + ".zones is empty");
        e.zones = z.zones;
        if (!z.external) {
            const auto it = std::find(names.begin(), names.end(), z.zones);
            if (it == names.end()) return refuse(where + ".zones '" + z.zones + "' names no band of the result (set external for a grid of set_zones)");
            e.band = (int)(it - names.begin());
        }
        for (int x : z.cell_stats) {
            if (x < 0 || (size_t)x >= cfg.cell_stats.size()) return refuse(where + ".cell_stats: no cell_stats entry " + std::to_string(x));
            e.stats.push_back(x);
        }
        for (int h : z.histograms) {
            if (h < 0 || (size_t)h >= cfg.histograms.size()) return refuse(where + ".histograms: no histogram " + std::to_string(h));
            e.hists.push_back(h);
        }
        if (!z.own_percentiles) {
            if (z.percentiles.size() > (size_t)zn::kMaxPercentiles) return refuse(where + ".percentiles: more than 16 percentiles");
            for (float q : z.percentiles)
                if (!(q >= 0.0f && q <= 1.0f)) return refuse(where + ".percentiles: a percentile must lie in [0, 1]");
        }
        for (int h : z.histograms) e.q.push_back(percentiles_of(cfg, z, h));
        if (z.max_zones < 1 || z.max_zones > (int)zn::kMaxZone) return refuse(where + ".max_zones must be between 1 and 2^24");
        e.max_zones = z.max_zones;
        if (Status s = check_zone_column_names(where, "cells", columns_of(cfg, z)); !s.ok()) return s;
        plan->entries.push_back(std::move(e));
    }
    return Status::success();
}

namespace {
Status unknown_zones(const PipelineConfig& cfg, const std::string& name) {
    bool known = false;
    for (const auto& z : cfg.zonal) known = known || (z.external && z.zones == name);
    if (known) return Status::success();
    return Status::error(StatusCode::InvalidArgument, "pipeline: set_zones: '" + name + "' names no external label grid of this pipeline");
}
}  // namespace

Status store_zones(const PipelineConfig& cfg, const std::string& name, const PolygonSet& polygons, const RasterizeOptions& options,
                   MemoryLocation loc, void* stream, std::map<std::string, ZoneGrid>* grids) {
    Status s = unknown_zones(cfg, name);
    if (!s.ok()) return s;
    ZoneGrid g;
    s = g.band.allocate((size_t)cfg.grid.width * (size_t)cfg.grid.height * sizeof(float), loc);
    if (s.ok()) s = rasterize_into(polygons, cfg.grid, options, static_cast<float*>(g.band.data()), loc, stream);
    if (s.ok()) (*grids)[name] = std::move(g);
    return s;
}

Status store_zones(const PipelineConfig& cfg, const std::string& name, const Grid& grid, int band, MemoryLocation loc, void* stream,
                   std::map<std::string, ZoneGrid>* grids) {
    auto bad = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: set_zones: " + msg); };
    if (Status known = unknown_zones(cfg, name); !known.ok()) return known;
    if (band < 0 || band >= grid.num_bands()) return bad("band index outside the grid");
    if (grid.band_desc(band).dtype != DataType::Float32 || !grid.band_f32(band)) return bad("the label band must be Float32");
    if (grid.cols() != cfg.grid.width || grid.rows() != cfg.grid.height)
        return bad("the grid is " + std::to_string(grid.cols()) + " x " + std::to_string(grid.rows()) + ", the pipeline's is " +
                   std::to_string(cfg.grid.width) + " x " + std::to_string(cfg.grid.height));
    const size_t bytes = (size_t)grid.cols() * (size_t)grid.rows() * sizeof(float);
    ZoneGrid g;
    Status s = g.band.allocate(bytes, loc);
    if (s.ok()) s = copy_bytes(g.band.data(), loc, grid.band_f32(band), grid.location(), bytes, stream);
    if (s.ok() && (loc == MemoryLocation::Device || grid.location() == MemoryLocation::Device))
        s = hip_status(pcr_hip_stream_synchronize(stream));
    if (s.ok()) (*grids)[name] = std::move(g);
    return s;
}

Status zonal_table(const ZonalPlan::Entry& e, const CellStatsPlan& cstats, const HistogramPlan& hist, const ZonalInputs& in,
                   bool with_counts, ZonalTable* out) {
    *out = ZonalTable();
    const MemoryLocation loc = in.device ? MemoryLocation::Device : MemoryLocation::Host;
    const int W = in.width, H = in.rows;
    pcr_hip_stream st = in.stream;

    // Z: the one value the host has to see before it can size anything
    uint32_t Zmax = 0;
    Status s = Status::success();
    if (in.device) {
        Buffer d_max;
        if (!(s = d_max.allocate(sizeof(uint32_t), MemoryLocation::Device)).ok()) return s;
        s = hip_status(pcr_hip_zone_max(in.zones, W, H, W, static_cast<uint32_t*>(d_max.data()), st));
        if (s.ok()) s = copy_bytes(&Zmax, MemoryLocation::Host, d_max.data(), loc, sizeof(uint32_t), st);
        const Status ws = hip_status(pcr_hip_stream_synchronize(st));
        if (s.ok()) s = ws;
    } else {
        s = hip_status(pcr_hip_zone_max_host(in.zones, W, H, W, &Zmax));
    }
    if (!s.ok()) return s;
    if ((int64_t)Zmax > e.max_zones)
        return Status::error(StatusCode::OutOfRange, "pipeline: zonal: zone " + std::to_string(Zmax) + " of '" + e.zones +
                                                     "' is above max_zones = " + std::to_string(e.max_zones));
    const size_t Z = Zmax;
    ZoneRowsInputs rows;
    for (size_t k = 0; k < e.stats.size(); ++k) {
        const CellStatsEntry& ce = cstats.entries[(size_t)e.stats[k]];
        rows.stats.push_back({ce.value_channel, nullptr, nullptr, nullptr, ce.origin, ce.resolution, ce.ddof});
    }
    for (size_t k = 0; k < e.hists.size(); ++k) {
        const HistogramEntry& he = hist.entries[(size_t)e.hists[k]];
        rows.hists.push_back({he.value_channel, nullptr, he.bins, he.lo, he.w, e.q[k]});
    }

    // the integer tables, zeroed, in one allocation of `loc` memory; the first stats fold counts the cells
    Arena a;
    if (Z != 0) {
        size_t bytes = Arena::padded(Z * 8);
        for (size_t k = 0; k < e.stats.size(); ++k) bytes += 3 * Arena::padded(Z * 8);
        for (size_t k = 0; k < e.hists.size(); ++k) bytes += Arena::padded(Z * (size_t)rows.hists[k].bins * 8);
        if (!(s = a.buf.allocate(bytes, loc)).ok()) return s;
        if (in.device) s = hip_status(pcr_hip_memset(a.buf.data(), 0, bytes, st));
        else std::memset(a.buf.data(), 0, bytes);
        if (!s.ok()) return s;

        const pcr_hip_zone_fold_params fold{1, 0};
        auto fold_stats = [&](const ZonalInputs::Stat& p, unsigned long long* cells, unsigned long long* n, long long* s1, unsigned long long* s2) {
            return hip_status(in.device ? pcr_hip_zone_fold_stats(in.zones, W, H, W, p.n, p.s1, p.s2, W, Zmax, &fold, cells, n, s1, s2, st)
                                        : pcr_hip_zone_fold_stats_host(in.zones, W, H, W, p.n, p.s1, p.s2, W, Zmax, &fold, cells, n, s1, s2));
        };
        unsigned long long* cells = a.take<unsigned long long>(Z);
        rows.count = cells;
        if (e.stats.empty()) s = fold_stats({nullptr, nullptr, nullptr}, cells, nullptr, nullptr, nullptr);       // (cells alone)
        for (size_t k = 0; k < e.stats.size() && s.ok(); ++k) {
            unsigned long long* n = a.take<unsigned long long>(Z);
            long long* s1 = a.take<long long>(Z);
            unsigned long long* s2 = a.take<unsigned long long>(Z);
            s = fold_stats(in.stats[(size_t)e.stats[k]], k == 0 ? cells : nullptr, n, s1, s2);
            rows.stats[k].n = n;
            rows.stats[k].s1 = s1;
            rows.stats[k].s2 = s2;
        }
        for (size_t k = 0; k < e.hists.size() && s.ok(); ++k) {
            const int bins = rows.hists[k].bins;
            const uint32_t* cube = in.cubes[(size_t)e.hists[k]];
            unsigned long long* counts = a.take<unsigned long long>(Z * (size_t)bins);
            const int64_t plane = (int64_t)W * H;
            s = hip_status(in.device ? pcr_hip_zone_fold_hist(in.zones, W, H, W, cube, bins, W, plane, Zmax, &fold, counts, st)
                                     : pcr_hip_zone_fold_hist_host(in.zones, W, H, W, cube, bins, W, plane, Zmax, &fold, counts));
            rows.hists[k].counts = counts;
        }
        if (!s.ok()) {
            if (in.device) (void)pcr_hip_stream_synchronize(st);     // (the arena is released behind what was enqueued)
            return s;
        }
    }
    return zone_rows(loc, st, Z, rows, with_counts, out->zone, out->cells, out->stats, out->hists);
}

}  // namespace detail
}  // namespace pcr
