// pipeline_common.cpp -- what the engines behind pcr::Pipeline share: the cloud checks, the filter plan and its sweep on the
// device, the grouping plan, `.pcrt` tile files of a window of state planes (see pipeline_common.h).
#include "pipeline_common.h"

#include "buffer.h"
#include "polygons.h"
#include "sample_grid.h"

#include "pcr/core/point_cloud.h"
#include "pcr/core/reproject.h"
#include "pcr/io/tile_state_io.h"

#include <algorithm>
#include <filesystem>

namespace pcr {
namespace detail {

Status validate_cloud(const PipelineConfig& cfg, const PointCloud& cloud, size_t max_set, size_t max_predicates) {
    // (a surface or polygon channel is a Float32 channel the pipeline derives itself: validate_surfaces and
    // validate_polygon_channels have checked it)
    auto derived = [&cfg](const std::string& name) { return derived_channel(cfg, name); };
    auto check_filter = [&](const FilterSpec& filter) -> Status {
        for (const auto& pr : filter.predicates) {
            if (derived(pr.channel_name)) continue;
            if (!cloud.channel_data(pr.channel_name))
                return Status::error(StatusCode::InvalidArgument, "filter_points: channel not found: " + pr.channel_name);
            const ChannelDesc* d = cloud.channel(pr.channel_name);
            if (!d || d->dtype != DataType::Float32)
                return Status::error(StatusCode::InvalidArgument, "filter_points: only Float32 channels supported for filtering");
            if (max_set && pr.value_set.size() > max_set)
                return Status::error(StatusCode::InvalidArgument,
                                     "filter_points: value_set larger than " + std::to_string(max_set) + " entries is not supported on the device");
        }
        return Status::success();
    };
    Status fs = check_filter(cfg.filter);
    if (!fs.ok()) return fs;
    if (max_predicates && cfg.filter.predicates.size() > max_predicates)
        return Status::error(StatusCode::InvalidArgument, "filter_points: more than " + std::to_string(max_predicates) + " predicates");
    for (const auto& r : cfg.reductions)                       // ReductionSpec::filter: the same checks, the same messages
        if (!(fs = check_filter(r.filter)).ok()) return fs;
    for (const auto& h : cfg.histograms) {                     // PipelineConfig::histograms: like a reduction's filter and value
        if (!(fs = check_filter(h.filter)).ok()) return fs;
        if (derived(h.value_channel)) continue;
        if (!cloud.channel_data(h.value_channel))
            return Status::error(StatusCode::InvalidArgument, "pipeline: histogram value channel not found: " + h.value_channel);
        const ChannelDesc* d = cloud.channel(h.value_channel);
        if (!d || d->dtype != DataType::Float32)
            return Status::error(StatusCode::InvalidArgument, "pipeline: histogram value channel must be Float32");
    }
    for (const auto& e : cfg.extremes) {                       // PipelineConfig::extremes: likewise
        if (!(fs = check_filter(e.filter)).ok()) return fs;
        if (derived(e.value_channel)) continue;
        if (!cloud.channel_data(e.value_channel))
            return Status::error(StatusCode::InvalidArgument, "pipeline: extremes value channel not found: " + e.value_channel);
        const ChannelDesc* d = cloud.channel(e.value_channel);
        if (!d || d->dtype != DataType::Float32)
            return Status::error(StatusCode::InvalidArgument, "pipeline: extremes value channel must be Float32");
    }
    for (const auto& c : cfg.cell_stats) {                     // PipelineConfig::cell_stats: likewise
        if (!(fs = check_filter(c.filter)).ok()) return fs;
        if (derived(c.value_channel)) continue;
        if (!cloud.channel_data(c.value_channel))
            return Status::error(StatusCode::InvalidArgument, "pipeline: cell_stats value channel not found: " + c.value_channel);
        const ChannelDesc* d = cloud.channel(c.value_channel);
        if (!d || d->dtype != DataType::Float32)
            return Status::error(StatusCode::InvalidArgument, "pipeline: cell_stats value channel must be Float32");
    }
    for (const auto& z : cfg.point_zonal) {                    // PipelineConfig::point_zonal: its specs' filters likewise (the channels:
        for (const auto& c : z.cell_stats)                     // validate_point_zonal)
            if (!(fs = check_filter(c.filter)).ok()) return fs;
        for (const auto& h : z.histograms)
            if (!(fs = check_filter(h.filter)).ok()) return fs;
    }
    for (const auto& r : cfg.reductions) {
        if (!derived(r.value_channel)) {
            if (!cloud.channel_data(r.value_channel))
                return Status::error(StatusCode::InvalidArgument, "pipeline: value channel not found: " + r.value_channel);
            const ChannelDesc* d = cloud.channel(r.value_channel);
            if (!d || d->dtype != DataType::Float32)
                return Status::error(StatusCode::InvalidArgument, "pipeline: value channel must be Float32");
        }
        if (r.glyph.type != GlyphType::Point && !glyph_reduction_ok(r.type))
            return Status::error(StatusCode::NotImplemented,
                "pipeline: glyph splatting only supports WeightedAverage, Average, Sum, or Count reduction types");
        if (is_select(r.type) && !derived(r.timestamp_channel)) {
            if (!cloud.channel_data(r.timestamp_channel))
                return Status::error(StatusCode::InvalidArgument, "pipeline: timestamp channel not found: " + r.timestamp_channel);
            const ChannelDesc* t = cloud.channel(r.timestamp_channel);
            if (!t || t->dtype != DataType::Float32)
                return Status::error(StatusCode::InvalidArgument, "pipeline: timestamp channel must be Float32");
        }
    }
    return Status::success();
}

Status plan_filters(const PipelineConfig& cfg, FilterPlan* out) {
    *out = FilterPlan{};
    out->classes.emplace_back();
    auto class_for = [out](const FilterSpec& filter) {
        int cls = 0;
        if (!filter.empty()) {
            for (size_t k = 1; k < out->classes.size() && !cls; ++k)
                if (same_filter(out->classes[k], filter)) cls = (int)k;
            if (!cls) {
                out->classes.push_back(filter);
                cls = (int)out->classes.size() - 1;
            }
        }
        return cls;
    };
    for (const auto& r : cfg.reductions) out->class_of.push_back(class_for(r.filter));
    for (const auto& h : cfg.histograms) out->hist_class_of.push_back(class_for(h.filter));   // (a histogram's filter is one more class)
    for (const auto& e : cfg.extremes) out->ext_class_of.push_back(class_for(e.filter));      // (and so is an extremes entry's)
    for (const auto& c : cfg.cell_stats) out->stat_class_of.push_back(class_for(c.filter));   // (and a cell-stats entry's)
    for (const auto& z : cfg.point_zonal) {                                                   // (and every spec's of a point-zonal entry)
        out->pz_stat_class_of.emplace_back();
        out->pz_hist_class_of.emplace_back();
        for (const auto& c : z.cell_stats) out->pz_stat_class_of.back().push_back(class_for(c.filter));
        for (const auto& h : z.histograms) out->pz_hist_class_of.back().push_back(class_for(h.filter));
    }
    if (out->classes.size() - 1 > kMaxSpecFilters)
        return Status::error(StatusCode::InvalidArgument, "pipeline: more than " + std::to_string(kMaxSpecFilters) +
                                                          " distinct reduction filters in one pipeline");
    for (size_t k = 1; k < out->classes.size(); ++k)
        if (cfg.filter.predicates.size() + out->classes[k].predicates.size() > PCR_HIP_MAX_FILTER_PREDICATES)
            return Status::error(StatusCode::InvalidArgument,
                "pipeline: a reduction filter and the pipeline's filter together hold more than " +
                std::to_string(PCR_HIP_MAX_FILTER_PREDICATES) + " predicates");
    auto place = [out](const FilterPredicate& pr) {
        for (size_t t = 0; t < out->table.size(); ++t)
            if (same_predicate(out->table[t], pr)) return t;
        out->table.push_back(pr);
        return out->table.size() - 1;
    };
    std::vector<std::vector<size_t>> at(out->classes.size());
    for (const auto& pr : cfg.filter.predicates) at[0].push_back(place(pr));
    for (size_t k = 1; k < out->classes.size(); ++k) {
        at[k] = at[0];
        for (const auto& pr : out->classes[k].predicates) at[k].push_back(place(pr));
    }
    if (out->table.size() > PCR_HIP_MAX_CLASS_PREDICATES) {
        if (out->any())
            return Status::error(StatusCode::InvalidArgument, "pipeline: more than " + std::to_string(PCR_HIP_MAX_CLASS_PREDICATES) +
                                                              " distinct filter predicates in one pipeline");
        out->table.clear();                // PipelineConfig::filter alone: no bit for every predicate, no table, and no refusal here
        return Status::success();
    }
    for (const auto& list : at) {
        uint32_t w = 0;
        for (size_t t : list) w |= 1u << t;
        out->words.push_back(w);
    }
    return Status::success();
}

Status marshal_predicates(const FilterSpec& filter, const ChannelLookup& channel, std::vector<pcr_hip_predicate>* out) {
    out->assign(filter.predicates.size(), pcr_hip_predicate{});
    for (size_t k = 0; k < out->size(); ++k) {
        const FilterPredicate& pr = filter.predicates[k];
        pcr_hip_predicate& hp = (*out)[k];
        Status s = channel(pr.channel_name, &hp.d_channel);
        if (!s.ok()) return s;
        hp.op = static_cast<int32_t>(pr.op);
        hp.value = pr.value;
        hp.set_size = static_cast<int32_t>(pr.value_set.size());
        for (size_t j = 0; j < pr.value_set.size(); ++j) hp.set[j] = pr.value_set[j];
    }
    return Status::success();
}

namespace {
constexpr size_t kSweepHeader = 128;                                   // the survivor counts, ahead of the masks
size_t sweep_stride(size_t n) { return (n + 15) & ~(size_t)15; }
// classes that get a mask: all of them, class 0 only when there is a PipelineConfig::filter
size_t first_masked(const FilterPlan& plan) { return !plan.words.empty() && plan.words[0] ? 0 : 1; }
}  // namespace

size_t filter_stage_bytes(const FilterPlan& plan, size_t n) {
    const size_t masked = plan.classes.size() - first_masked(plan);
    return masked ? kSweepHeader + masked * sweep_stride(n) : 0;
}

Status sweep_filter_classes(const FilterPlan& plan, const ChannelLookup& channel, size_t n, void* d_buffer, pcr_hip_stream stream,
                            std::vector<const uint8_t*>* masks, size_t* kept) {
    const size_t first = first_masked(plan), n_cls = plan.classes.size(), stride = sweep_stride(n);
    masks->assign(n_cls, nullptr);
    *kept = n;
    if (first == n_cls) return Status::success();
    FilterSpec table;
    table.predicates = plan.table;
    std::vector<pcr_hip_predicate> preds;
    Status s = marshal_predicates(table, channel, &preds);
    if (!s.ok()) return s;
    uint8_t* const base = static_cast<uint8_t*>(d_buffer) + kSweepHeader;
    auto* const d_counts = static_cast<unsigned long long*>(d_buffer);
    for (size_t c = first; c < n_cls; c += PCR_HIP_MAX_FILTER_CLASSES) {
        const int m = (int)std::min<size_t>(PCR_HIP_MAX_FILTER_CLASSES, n_cls - c);
        s = hip_status(pcr_hip_filter_classes(preds.data(), (int)preds.size(), plan.words.data() + c, m, n, base + (c - first) * stride,
                                              stride, c == 0 ? d_counts : nullptr, stream));
        if (!s.ok()) return s;
        for (int k = 0; k < m; ++k) (*masks)[c + (size_t)k] = base + (c - first + (size_t)k) * stride;
    }
    if (first != 0) return Status::success();
    unsigned long long h_count = 0;
    if (!(s = hip_status(pcr_hip_memcpy_d2h(&h_count, d_counts, sizeof h_count, stream))).ok()) return s;
    if (!(s = hip_status(pcr_hip_stream_synchronize(stream))).ok()) return s;
    *kept = (size_t)h_count;
    return Status::success();
}

GroupPlan plan_groups(const PipelineConfig& cfg) {
    GroupPlan plan;
    FilterPlan filters;
    (void)plan_filters(cfg, &filters);                  // (the classes are numbered whatever it refuses)
    std::vector<const ReductionSpec*> first;
    for (size_t ri = 0; ri < cfg.reductions.size(); ++ri) {
        const ReductionSpec& r = cfg.reductions[ri];
        int gi = -1;
        for (size_t k = 0; k < first.size(); ++k)
            if (same_group(*first[k], r)) gi = (int)k;
        if (gi < 0) {
            first.push_back(&r);
            gi = (int)first.size() - 1;
            GroupSpec gs;
            gs.value_channel = r.value_channel;
            gs.glyph = r.glyph;
            gs.select = is_select(r.type);
            if (gs.select) gs.key_channel = r.timestamp_channel;
            gs.filter = r.filter;
            gs.cls = filters.class_of[ri];
            plan.groups.push_back(gs);
        }
        // (a glyph reduction of an unsupported type is refused at ingest, as in the reference: it still gets its planes)
        plan.groups[(size_t)gi].mask |= planes_for(r.type);
        Output o;
        o.group = gi;
        o.type = r.type;
        o.band_name = default_band_name(r);
        plan.outputs.push_back(o);
    }
    for (size_t h = 0; h < cfg.histograms.size(); ++h)
        for (size_t j = 0; j < cfg.histograms[h].percentiles.size(); ++j) {
            Output o;
            o.group = -1;
            o.type = ReductionType::Max;
            o.band_name = histogram_band_name(cfg.histograms[h], j);
            o.hist = (int)h;
            o.q = (int)j;
            plan.outputs.push_back(o);
        }
    for (size_t i = 0; i < cfg.extremes.size(); ++i) {
        Output o;
        o.group = -1;
        o.type = cfg.extremes[i].side == ExtremeSide::Highest ? ReductionType::Max : ReductionType::Min;
        o.band_name = extremes_band_name(cfg.extremes[i]);
        o.ext = (int)i;
        plan.outputs.push_back(o);
    }
    for (size_t i = 0; i < cfg.cell_stats.size(); ++i)
        for (size_t j = 0; j < cfg.cell_stats[i].products.size(); ++j) {
            Output o;
            o.group = -1;
            o.type = cfg.cell_stats[i].products[j] == CellStat::Mean ? ReductionType::Average : ReductionType::Sum;
            o.band_name = cell_stats_band_name(cfg.cell_stats[i], j);
            o.stat = (int)i;
            o.product = (int)j;
            plan.outputs.push_back(o);
        }
    return plan;
}

Status plan_reprojection(const PipelineConfig& cfg, const PointCloud& cloud, Reprojection* out) {
    *out = Reprojection{};
    if (!cfg.auto_reproject) return Status::success();
    const CRS& dst = cfg.grid.crs.is_valid() ? cfg.grid.crs : cfg.target_crs;
    const int from = crs_epsg(cloud.crs()), to = crs_epsg(dst);
    if (from == 0 || to == 0 || from == to) return Status::success();
    if (pcr_hip_crs_from_epsg(from, &out->src) != PCR_HIP_OK || pcr_hip_crs_from_epsg(to, &out->dst) != PCR_HIP_OK)
        return Status::error(StatusCode::CrsError, "pipeline: cannot reproject the cloud from EPSG:" + std::to_string(from) +
                             " to EPSG:" + std::to_string(to) + " (" + pcr_hip_last_error() + "); nothing was accumulated");
    out->needed = true;
    out->dst_crs = dst;
    return Status::success();
}

std::string reduction_state_dir(const std::string& dir, size_t r, size_t n_outputs) {
    return n_outputs == 1 ? dir : dir + "/reduction_" + std::to_string(r);
}

namespace {
struct TileRect { int c0, r0, nc, nr; bool inside; };

TileRect tile_rect(const GridConfig& g, const StateWindow& w, int tx, int ty) {
    TileRect t;
    t.c0 = tx * g.tile_width;
    t.r0 = ty * g.tile_height;
    t.nc = std::min(g.tile_width, g.width - t.c0);
    t.nr = std::min(g.tile_height, g.height - t.r0);
    const int lo = w.own_row0 >= 0 ? w.own_row0 : w.row0, hi = w.own_row0 >= 0 ? w.own_row1 : w.row0 + w.rows;
    t.inside = t.r0 >= lo && t.r0 + t.nr <= hi && t.r0 >= w.row0 && t.r0 + t.nr <= w.row0 + w.rows;
    return t;
}
}  // namespace

Status write_state_tiles(const GridConfig& g, const std::vector<Output>& outputs, const StateWindow& w,
                         const std::vector<uint32_t>& touched, const std::string& dir, std::vector<std::string>* written) {
    const int tiles_x = (g.width + g.tile_width - 1) / g.tile_width;
    const int tiles_y = (g.height + g.tile_height - 1) / g.tile_height;
    std::error_code ec;
    std::vector<float> buf;
    for (size_t r = 0; r < outputs.size(); ++r) {
        const std::string rdir = reduction_state_dir(dir, r, outputs.size());
        std::filesystem::create_directories(rdir, ec);
        if (ec) return Status::error(StatusCode::IoError, "pipeline: cannot create " + rdir);
        int pl[2];
        const int k = state_planes_of(outputs[r].type, pl);
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                if (!touched[(size_t)ty * tiles_x + tx]) continue;          // only tiles that have state
                const TileRect t = tile_rect(g, w, tx, ty);
                if (!t.inside) continue;
                buf.resize((size_t)k * t.nc * t.nr);
                for (int f = 0; f < k; ++f) {
                    const float* plane = w.plane(outputs[r].group, pl[f]);
                    if (!plane) return Status::error(StatusCode::InvalidArgument, "pipeline: a reduction's state plane is missing");
                    for (int y = 0; y < t.nr; ++y)
                        std::copy_n(plane + (size_t)(t.r0 - w.row0 + y) * g.width + t.c0, t.nc, buf.data() + ((size_t)f * t.nr + y) * t.nc);
                }
                TileIndex ti;
                ti.row = ty;
                ti.col = tx;
                const std::string path = tile_state_filename(rdir, ti);
                Status s = write_tile_state(path, ti, t.nc, t.nr, k, outputs[r].type, buf.data());
                if (!s.ok()) return s;
                if (written) written->push_back(path);
            }
    }
    return Status::success();
}

Status read_state_tiles(const GridConfig& g, const std::vector<Output>& outputs, const StateWindow& w,
                        std::vector<uint32_t>& touched, const std::string& dir, size_t* loaded) {
    const int tiles_x = (g.width + g.tile_width - 1) / g.tile_width;
    const int tiles_y = (g.height + g.tile_height - 1) / g.tile_height;
    // rows this window takes from the files: its own rows (a shard never loads into its apron), else the whole window.  A
    // tile that the range only CUTS is read whole and its rows inside the range are taken: a row-block shard resumes from any
    // checkpoint of the grid, whoever wrote it.
    const int lo = w.own_row0 >= 0 ? std::max(w.own_row0, w.row0) : w.row0;
    const int hi = w.own_row0 >= 0 ? std::min(w.own_row1, w.row0 + w.rows) : w.row0 + w.rows;
    std::vector<float> buf;
    size_t taken = 0;
    for (size_t r = 0; r < outputs.size(); ++r) {
        const std::string rdir = reduction_state_dir(dir, r, outputs.size());
        int pl[2];
        const int k = state_planes_of(outputs[r].type, pl);
        for (int ty = 0; ty < tiles_y; ++ty)
            for (int tx = 0; tx < tiles_x; ++tx) {
                const TileRect t = tile_rect(g, w, tx, ty);
                const int y0 = std::max(t.r0, lo), y1 = std::min(t.r0 + t.nr, hi);
                if (y0 >= y1) continue;
                TileIndex ti;
                ti.row = ty;
                ti.col = tx;
                const std::string path = tile_state_filename(rdir, ti);
                std::error_code ec;
                if (!std::filesystem::exists(path, ec)) continue;
                TileIndex ft;
                int fc = 0, fr = 0, fk = 0;
                ReductionType ftype;
                if (!read_tile_state_header(path, ft, fc, fr, fk, ftype).ok()) continue;
                if (fc != t.nc || fr != t.nr || fk != k || ftype != outputs[r].type || ft.row != ty || ft.col != tx) continue;
                buf.resize((size_t)k * t.nc * t.nr);
                if (!read_tile_state(path, ft, fc, fr, fk, ftype, buf.data()).ok()) continue;
                for (int f = 0; f < k; ++f) {
                    float* plane = w.plane(outputs[r].group, pl[f]);
                    if (!plane) return Status::error(StatusCode::InvalidArgument, "pipeline: a reduction's state plane is missing");
                    for (int y = y0; y < y1; ++y)
                        std::copy_n(buf.data() + ((size_t)f * t.nr + (y - t.r0)) * t.nc, t.nc, plane + (size_t)(y - w.row0) * g.width + t.c0);
                }
                touched[(size_t)ty * tiles_x + tx] = 1;
                ++taken;
            }
    }
    if (loaded) *loaded = taken;
    return Status::success();
}

}  // namespace detail
}  // namespace pcr
