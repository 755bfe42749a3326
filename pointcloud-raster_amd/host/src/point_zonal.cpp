// point_zonal.cpp -- see point_zonal.h.
#include "point_zonal.h"

#include "pcr/core/point_cloud.h"
#include "polygons.h"
#include "sample_grid.h"
#include "zone_rows.h"

#include <algorithm>
#include <cstring>

namespace pcr {
namespace detail {

namespace {

// What zone_rows makes entry e's columns from: its specs, and with `t` (the entry's state) the integer tables.  t null: the
// columns' names alone.
ZoneRowsInputs rows_of(const PointZonalPlan::Entry& e, const unsigned long long* t) {
    ZoneRowsInputs r;
    if (t) r.count = t + e.points_at();
    for (size_t k = 0; k < e.stats.size(); ++k) {
        const CellStatsEntry& c = e.stats[k];
        const unsigned long long* n = t ? t + e.stat_at(k) : nullptr;
        r.stats.push_back({c.value_channel, n, t ? reinterpret_cast<const long long*>(n + e.Z) : nullptr, t ? n + 2 * (size_t)e.Z : nullptr,
                           c.origin, c.resolution, c.ddof});
    }
    for (size_t k = 0; k < e.hists.size(); ++k) {
        const HistogramEntry& h = e.hists[k];
        r.hists.push_back({h.value_channel, t ? t + e.hist_at(k) : nullptr, h.bins, h.lo, h.w, h.q});
    }
    return r;
}

// One entry's refusals and its plan; `stat_cls` / `hist_cls`: the specs' filter classes (empty: class 0).
Status plan_entry(const PointZonalConfig& z, const std::string& where, const std::vector<int>& stat_cls, const std::vector<int>& hist_cls,
                  PointZonalPlan::Entry* out) {
    PointZonalPlan::Entry e;
    if (z.label_channel.empty()) return refuse(where + ".label_channel is empty");
    e.label = z.label_channel;
    if (z.cell_stats.size() > kMaxPointZonalSpecs) return refuse(where + ": more than 4 cell_stats specs");
    if (z.histograms.size() > kMaxPointZonalSpecs) return refuse(where + ": more than 4 histograms");
    if (z.max_zones < 1 || z.max_zones > (int)pcrhip::pzonal::kMaxZone) return refuse(where + ".max_zones must be between 1 and 2^24");
    e.Z = (uint32_t)z.max_zones;
    for (size_t k = 0; k < z.cell_stats.size(); ++k) {               // the per-spec refusals of PipelineConfig::cell_stats
        const CellStatsConfig& c = z.cell_stats[k];
        const std::string at = where + ".cell_stats[" + std::to_string(k) + "]";
        Status s = check_cell_stats_value(c, at);
        if (s.ok()) s = check_cell_stats_ddof(c, at);
        if (!s.ok()) return s;
        e.stats.push_back(cell_stats_entry(c, k < stat_cls.size() ? stat_cls[k] : 0));
    }
    for (size_t k = 0; k < z.histograms.size(); ++k) {               // ... and of PipelineConfig::histograms
        const HistogramConfig& h = z.histograms[k];
        if (Status s = check_histogram_spec(h, where + ".histograms[" + std::to_string(k) + "]"); !s.ok()) return s;
        e.hists.push_back(histogram_entry(h, k < hist_cls.size() ? hist_cls[k] : 0));
    }
    if (Status s = check_zone_column_names(where, "points", rows_of(e, nullptr)); !s.ok()) return s;
    *out = std::move(e);
    return Status::success();
}

}  // namespace

size_t PointZonalPlan::Entry::hist_at(size_t k) const {
    size_t at = 2 + (size_t)Z * (1 + 3 * stats.size());
    for (size_t j = 0; j < k; ++j) at += (size_t)Z * (size_t)hists[j].bins;
    return at;
}
size_t PointZonalPlan::Entry::words() const { return hist_at(hists.size()); }

Status plan_point_zonal(const PipelineConfig& cfg, const FilterPlan& filters, PointZonalPlan* plan) {
    *plan = PointZonalPlan();
    if (cfg.point_zonal.empty()) return Status::success();
    if (cfg.point_zonal.size() > kMaxPointZonal) return refuse("point_zonal: more than 4 entries");
    for (size_t i = 0; i < cfg.point_zonal.size(); ++i) {
        PointZonalPlan::Entry e;
        static const std::vector<int> none;
        Status s = plan_entry(cfg.point_zonal[i], "point_zonal[" + std::to_string(i) + "]",
                              i < filters.pz_stat_class_of.size() ? filters.pz_stat_class_of[i] : none,
                              i < filters.pz_hist_class_of.size() ? filters.pz_hist_class_of[i] : none, &e);
        if (!s.ok()) return s;
        plan->entries.push_back(std::move(e));
    }
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0)
        return refuse("point_zonal tables are not supported on a row-block shard: a shard ingests only the points of its rows");
    return Status::success();
}

size_t point_zonal_state_bytes(const PipelineConfig& cfg) {
    size_t bytes = 0;
    for (const auto& z : cfg.point_zonal) {
        size_t row = 8 + 24 * z.cell_stats.size();
        for (const auto& h : z.histograms) row += 8 * (size_t)std::max(h.bins, 0);
        bytes += 16 + (size_t)std::max(z.max_zones, 0) * row;
    }
    return bytes;
}

Status point_zonal_out_of_core_error() {
    return refuse("point_zonal tables need the state in HBM: the grid and the tables do not fit gpu_memory_budget and the pipeline would "
                  "run out of core");
}

Status point_zonal_checkpoint_error() {
    return Status::error(StatusCode::NotImplemented,
                         "pipeline: checkpoints do not carry the point zonal tables yet: save_state, load_state and resume are "
                         "refused while PipelineConfig::point_zonal is not empty");
}

Status validate_point_zonal(const PipelineConfig& cfg, const PointCloud& cloud) {
    auto f32 = [&](const std::string& name, const std::string& what) -> Status {
        if (derived_channel(cfg, name)) return Status::success();
        if (!cloud.channel_data(name)) return Status::error(StatusCode::InvalidArgument, "pipeline: point_zonal " + what + " channel not found: " + name);
        const ChannelDesc* d = cloud.channel(name);
        if (!d || d->dtype != DataType::Float32)
            return Status::error(StatusCode::InvalidArgument, "pipeline: point_zonal " + what + " channel must be Float32: " + name);
        return Status::success();
    };
    for (const auto& z : cfg.point_zonal) {
        Status s = f32(z.label_channel, "label");
        for (const auto& c : z.cell_stats) {
            if (s.ok()) s = f32(c.value_channel, "value");
            for (const auto& pr : c.filter.predicates)
                if (s.ok()) s = f32(pr.channel_name, "filter");
        }
        for (const auto& h : z.histograms) {
            if (s.ok()) s = f32(h.value_channel, "value");
            for (const auto& pr : h.filter.predicates)
                if (s.ok()) s = f32(pr.channel_name, "filter");
        }
        if (!s.ok()) return s;
    }
    return Status::success();
}

Status PointZonalState::allocate(const PointZonalPlan& plan, MemoryLocation loc, void* stream) {
    tables.clear();
    tables.resize(plan.entries.size());
    for (size_t i = 0; i < tables.size(); ++i) {
        const size_t bytes = plan.entries[i].words() * 8;
        Status s = tables[i].allocate(bytes, loc);
        if (!s.ok()) return s;
        if (loc == MemoryLocation::Device) s = hip_status(pcr_hip_memset(tables[i].data(), 0, bytes, stream));
        else std::memset(tables[i].data(), 0, bytes);
        if (!s.ok()) return s;
    }
    return Status::success();
}

Status point_zonal_fold(const PointZonalPlan& plan, PointZonalState& state, const PointZonalInputs& in) {
    if (in.n == 0) return Status::success();
    using u64 = unsigned long long;
    const pcr_hip_point_fold_params auto_path{0, 0};
    for (size_t i = 0; i < plan.entries.size(); ++i) {
        const PointZonalPlan::Entry& e = plan.entries[i];
        u64* t = static_cast<u64*>(state.tables[i].data());
        const float* label = nullptr;
        Status s = in.channel(e.label, &label);
        if (!s.ok()) return s;
        if (!label) return Status::error(StatusCode::InvalidArgument, "pipeline: point_zonal label channel not found: " + e.label);
        auto stats = [&](const uint8_t* mask, const float* v, const CellStatsEntry* sp, size_t k, bool with_points) {
            u64* pts = with_points ? t + e.points_at() : nullptr;
            u64* inf = with_points ? t : nullptr;
            u64* zn = sp ? t + e.stat_at(k) : nullptr;
            long long* zs1 = sp ? reinterpret_cast<long long*>(zn + e.Z) : nullptr;
            u64* zs2 = sp ? zn + 2 * (size_t)e.Z : nullptr;
            const double origin = sp ? sp->origin : 0.0, inv_res = sp ? sp->inv_res : 1.0;
            return hip_status(in.device ? pcr_hip_point_fold_stats(label, mask, v, in.n, origin, inv_res, e.Z, &auto_path, pts, zn, zs1, zs2,
                                                                   inf, in.stream)
                                        : pcr_hip_point_fold_stats_host(label, mask, v, in.n, origin, inv_res, e.Z, &auto_path, pts, zn, zs1,
                                                                        zs2, inf));
        };
        // `points` and the info words are PipelineConfig::filter's survivors': they ride on the first stats spec of class 0, or
        // take a pass of their own (label and mask alone)
        size_t rider = e.stats.size();
        for (size_t k = 0; k < e.stats.size() && rider == e.stats.size(); ++k)
            if (e.stats[k].cls == 0) rider = k;
        if (rider == e.stats.size() && !(s = stats(in.mask(0), nullptr, nullptr, 0, true)).ok()) return s;
        for (size_t k = 0; k < e.stats.size(); ++k) {
            const float* v = nullptr;
            if (!(s = in.channel(e.stats[k].value_channel, &v)).ok()) return s;
            if (!v) return Status::error(StatusCode::InvalidArgument, "pipeline: point_zonal value channel not found: " + e.stats[k].value_channel);
            if (!(s = stats(in.mask(e.stats[k].cls), v, &e.stats[k], k, k == rider)).ok()) return s;
        }
        for (size_t k = 0; k < e.hists.size(); ++k) {
            const HistogramEntry& h = e.hists[k];
            const float* v = nullptr;
            if (!(s = in.channel(h.value_channel, &v)).ok()) return s;
            if (!v) return Status::error(StatusCode::InvalidArgument, "pipeline: point_zonal value channel not found: " + h.value_channel);
            u64* counts = t + e.hist_at(k);
            s = hip_status(in.device ? pcr_hip_point_fold_hist(label, in.mask(h.cls), v, in.n, h.bins, h.lo, h.inv_w, e.Z, &auto_path, counts,
                                                               nullptr, in.stream)
                                     : pcr_hip_point_fold_hist_host(label, in.mask(h.cls), v, in.n, h.bins, h.lo, h.inv_w, e.Z, &auto_path,
                                                                    counts, nullptr));
            if (!s.ok()) return s;
        }
    }
    return Status::success();
}

Status point_zonal_table(const PointZonalPlan::Entry& e, const Buffer& table, void* st, bool with_counts, PointZonalTable* out) {
    *out = PointZonalTable();
    using u64 = unsigned long long;
    const MemoryLocation loc = table.location();
    const u64* t = static_cast<const u64*>(table.data());

    // the info words: what the host has to see before it can size anything
    u64 info[2] = {0, 0};
    Status s = copy_bytes(info, MemoryLocation::Host, t, loc, sizeof info, st);
    if (loc == MemoryLocation::Device) {
        const Status ws = hip_status(pcr_hip_stream_synchronize(st));
        if (s.ok()) s = ws;
    }
    if (!s.ok()) return s;
    if (info[1] != 0)
        return Status::error(StatusCode::OutOfRange, "pipeline: point_zonal: " + std::to_string(info[1]) + " points of '" + e.label +
                                                     "' carry a zone above max_zones = " + std::to_string(e.Z));
    return zone_rows(loc, st, (size_t)info[0], rows_of(e, t), with_counts, out->zone, out->points, out->stats, out->hists);
}

}  // namespace detail

Status point_zonal(const PointCloud& cloud, const PointZonalConfig& config, PointZonalTable* out, bool with_counts) {
    if (!out) return Status::error(StatusCode::InvalidArgument, "point_zonal: null table");
    for (const auto& c : config.cell_stats)
        if (!c.filter.empty()) return Status::error(StatusCode::InvalidArgument, "point_zonal: a spec's filter needs a pipeline (PipelineConfig::point_zonal)");
    for (const auto& h : config.histograms)
        if (!h.filter.empty()) return Status::error(StatusCode::InvalidArgument, "point_zonal: a spec's filter needs a pipeline (PipelineConfig::point_zonal)");
    PipelineConfig cfg;
    cfg.point_zonal = {config};
    detail::FilterPlan filters;
    detail::PointZonalPlan plan;
    Status s = detail::plan_point_zonal(cfg, filters, &plan);
    if (s.ok()) s = detail::validate_point_zonal(cfg, cloud);
    if (!s.ok()) return s;
    const bool device = cloud.location() == MemoryLocation::Device;
    detail::PointZonalState state;
    if (!(s = state.allocate(plan, device ? MemoryLocation::Device : MemoryLocation::Host, nullptr)).ok()) return s;
    detail::PointZonalInputs in;
    in.device = device;
    in.n = cloud.count();
    in.channel = [&cloud](const std::string& name, const float** p) {
        *p = cloud.channel_f32(name);
        return Status::success();
    };
    in.mask = [](int) -> const uint8_t* { return nullptr; };
    if (!(s = detail::point_zonal_fold(plan, state, in)).ok()) return s;
    return detail::point_zonal_table(plan.entries[0], state.tables[0], nullptr, with_counts, out);
}

}  // namespace pcr
