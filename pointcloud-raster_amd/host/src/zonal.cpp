// zonal.cpp -- see zonal.h.
#include "zonal.h"

#include "pipeline_common.h"
#include "polygons.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace pcr {
namespace detail {

namespace zn = pcrhip::zonal;

namespace {

Status refuse(const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: " + msg); }

const std::vector<float>& percentiles_of(const PipelineConfig& cfg, const ZonalConfig& z, int h) {
    return z.own_percentiles ? cfg.histograms[(size_t)h].percentiles : z.percentiles;
}

}  // namespace

std::vector<std::string> zonal_column_names(const PipelineConfig& cfg, const ZonalConfig& z) {
    std::vector<std::string> names{"zone", "cells"};
    for (int x : z.cell_stats) {
        const std::string& ch = cfg.cell_stats[(size_t)x].value_channel;
        for (const char* suffix : {"_n", "_mean", "_var", "_std"}) names.push_back(ch + suffix);
    }
    for (int h : z.histograms) {
        const std::string& ch = cfg.histograms[(size_t)h].value_channel;
        names.push_back(ch + "_hist_n");
        for (float q : percentiles_of(cfg, z, h)) names.push_back(ch + "_p" + std::to_string(std::lround((double)q * 100.0)));
    }
    return names;
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
        std::vector<std::string> cols = zonal_column_names(cfg, z);
        std::sort(cols.begin(), cols.end());
        const auto dup = std::adjacent_find(cols.begin(), cols.end());
        if (dup != cols.end()) return refuse(where + ": column '" + *dup + "' appears twice");
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

namespace {

// The tables of one call in one allocation of `loc` memory, zeroed: pieces are handed out on 256 bytes.
struct Arena {
    Buffer buf;
    size_t used = 0;
    static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(static_cast<char*>(buf.data()) + used);
        used += padded(count * sizeof(T));
        return p;
    }
};

}  // namespace

Status zonal_table(const ZonalPlan::Entry& e, const CellStatsPlan& cstats, const HistogramPlan& hist, const ZonalInputs& in,
                   bool with_counts, ZonalTable* out) {
    *out = ZonalTable();
    const MemoryLocation loc = in.device ? MemoryLocation::Device : MemoryLocation::Host;
    const int W = in.width, H = in.rows;
    pcr_hip_stream st = in.stream;
    auto fetch = [&](void* dst, const void* src, size_t bytes) { return copy_bytes(dst, MemoryLocation::Host, src, loc, bytes, st); };

    // Z: the one value the host has to see before it can size anything
    uint32_t Zmax = 0;
    Status s = Status::success();
    if (in.device) {
        Buffer d_max;
        if (!(s = d_max.allocate(sizeof(uint32_t), MemoryLocation::Device)).ok()) return s;
        s = hip_status(pcr_hip_zone_max(in.zones, W, H, W, static_cast<uint32_t*>(d_max.data()), st));
        if (s.ok()) s = fetch(&Zmax, d_max.data(), sizeof(uint32_t));
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
    out->stats.resize(e.stats.size());
    out->hists.resize(e.hists.size());
    for (size_t k = 0; k < e.stats.size(); ++k) out->stats[k].channel = cstats.entries[(size_t)e.stats[k]].value_channel;
    for (size_t k = 0; k < e.hists.size(); ++k) {
        const HistogramEntry& he = hist.entries[(size_t)e.hists[k]];
        out->hists[k].channel = he.value_channel;
        out->hists[k].bins = he.bins;
        out->hists[k].q = e.q[k];
        out->hists[k].p.resize(e.q[k].size());
    }
    if (Z == 0) return Status::success();

    size_t bytes = Arena::padded(Z * 8);
    for (size_t k = 0; k < e.stats.size(); ++k) bytes += 3 * Arena::padded(Z * 8) + 3 * Arena::padded(Z * 4);
    for (size_t k = 0; k < e.hists.size(); ++k)
        bytes += Arena::padded(Z * (size_t)out->hists[k].bins * 8) + Arena::padded(Z * 8) + e.q[k].size() * Arena::padded(Z * 4);
    Arena a;
    if (!(s = a.buf.allocate(bytes, loc)).ok()) return s;
    if (in.device) s = hip_status(pcr_hip_memset(a.buf.data(), 0, bytes, st));
    else std::memset(a.buf.data(), 0, bytes);
    if (!s.ok()) return s;

    const pcr_hip_zone_fold_params fold{1, 0};
    unsigned long long* cells = a.take<unsigned long long>(Z);
    struct StatTables { unsigned long long* n; long long* s1; unsigned long long* s2; float *mean, *var, *sd; };
    struct HistTables { unsigned long long* counts; unsigned long long* n; std::vector<float*> p; };
    std::vector<StatTables> st_tab(e.stats.size());
    std::vector<HistTables> hi_tab(e.hists.size());
    if (e.stats.empty()) {                               // (cells alone)
        s = in.device ? hip_status(pcr_hip_zone_fold_stats(in.zones, W, H, W, nullptr, nullptr, nullptr, W, Zmax, &fold, cells, nullptr,
                                                           nullptr, nullptr, st))
                      : hip_status(pcr_hip_zone_fold_stats_host(in.zones, W, H, W, nullptr, nullptr, nullptr, W, Zmax, &fold, cells, nullptr,
                                                                nullptr, nullptr));
    }
    for (size_t k = 0; k < e.stats.size() && s.ok(); ++k) {
        const CellStatsEntry& ce = cstats.entries[(size_t)e.stats[k]];
        const ZonalInputs::Stat& p = in.stats[(size_t)e.stats[k]];
        StatTables& t = st_tab[k];
        t.n = a.take<unsigned long long>(Z);
        t.s1 = a.take<long long>(Z);
        t.s2 = a.take<unsigned long long>(Z);
        t.mean = a.take<float>(Z);
        t.var = a.take<float>(Z);
        t.sd = a.take<float>(Z);
        unsigned long long* c = k == 0 ? cells : nullptr;        // the first entry's fold counts the cells
        if (in.device) {
            s = hip_status(pcr_hip_zone_fold_stats(in.zones, W, H, W, p.n, p.s1, p.s2, W, Zmax, &fold, c, t.n, t.s1, t.s2, st));
            if (s.ok()) s = hip_status(pcr_hip_zone_rows_stats(t.n, t.s1, t.s2, Zmax, ce.origin, ce.resolution, ce.ddof, t.mean, t.var, t.sd, st));
        } else {
            s = hip_status(pcr_hip_zone_fold_stats_host(in.zones, W, H, W, p.n, p.s1, p.s2, W, Zmax, &fold, c, t.n, t.s1, t.s2));
            if (s.ok()) s = hip_status(pcr_hip_zone_rows_stats_host(t.n, t.s1, t.s2, Zmax, ce.origin, ce.resolution, ce.ddof, t.mean, t.var, t.sd));
        }
    }
    for (size_t k = 0; k < e.hists.size() && s.ok(); ++k) {
        const HistogramEntry& he = hist.entries[(size_t)e.hists[k]];
        const uint32_t* cube = in.cubes[(size_t)e.hists[k]];
        HistTables& t = hi_tab[k];
        t.counts = a.take<unsigned long long>(Z * (size_t)he.bins);
        t.n = a.take<unsigned long long>(Z);
        for (size_t j = 0; j < e.q[k].size(); ++j) t.p.push_back(a.take<float>(Z));
        const int64_t plane = (int64_t)W * H;
        const int nq = (int)e.q[k].size();
        if (in.device) {
            s = hip_status(pcr_hip_zone_fold_hist(in.zones, W, H, W, cube, he.bins, W, plane, Zmax, &fold, t.counts, st));
            if (s.ok()) s = hip_status(pcr_hip_zone_rows_percentiles(t.counts, he.bins, Zmax, he.lo, he.w, nq, e.q[k].data(), t.n, t.p.data(), st));
        } else {
            s = hip_status(pcr_hip_zone_fold_hist_host(in.zones, W, H, W, cube, he.bins, W, plane, Zmax, &fold, t.counts));
            if (s.ok()) s = hip_status(pcr_hip_zone_rows_percentiles_host(t.counts, he.bins, Zmax, he.lo, he.w, nq, e.q[k].data(), t.n, t.p.data()));
        }
    }

    // the table leaves
    out->zone.resize(Z);
    for (size_t k = 0; k < Z; ++k) out->zone[k] = (int32_t)(k + 1);
    out->cells.resize(Z);
    if (s.ok()) s = fetch(out->cells.data(), cells, Z * 8);
    for (size_t k = 0; k < e.stats.size() && s.ok(); ++k) {
        ZonalTable::StatColumns& c = out->stats[k];
        c.n.resize(Z);
        c.mean.resize(Z);
        c.var.resize(Z);
        c.stddev.resize(Z);
        s = fetch(c.n.data(), st_tab[k].n, Z * 8);
        if (s.ok()) s = fetch(c.mean.data(), st_tab[k].mean, Z * 4);
        if (s.ok()) s = fetch(c.var.data(), st_tab[k].var, Z * 4);
        if (s.ok()) s = fetch(c.stddev.data(), st_tab[k].sd, Z * 4);
    }
    for (size_t k = 0; k < e.hists.size() && s.ok(); ++k) {
        ZonalTable::HistColumns& c = out->hists[k];
        c.hist_n.resize(Z);
        s = fetch(c.hist_n.data(), hi_tab[k].n, Z * 8);
        if (with_counts) {
            c.counts.resize(Z * (size_t)c.bins);
            if (s.ok()) s = fetch(c.counts.data(), hi_tab[k].counts, c.counts.size() * 8);
        }
        for (size_t j = 0; j < c.p.size() && s.ok(); ++j) {
            c.p[j].resize(Z);
            s = fetch(c.p[j].data(), hi_tab[k].p[j], Z * 4);
        }
    }
    if (in.device) {
        const Status ws = hip_status(pcr_hip_stream_synchronize(st));     // (the arena is released behind the copies)
        if (s.ok()) s = ws;
    }
    if (!s.ok()) *out = ZonalTable();
    return s;
}

}  // namespace detail
}  // namespace pcr
