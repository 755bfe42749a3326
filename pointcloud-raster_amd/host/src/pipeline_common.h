// pipeline_common.h -- (internal) what the engines behind Pipeline share: which reductions exist, which planes they
// need, the grouping plan (which ReductionSpecs share a pass over the points, which bands come out), the filter stage (its plan
// and its one sweep on the device), and the `.pcrt` tile files of a state window.
#pragma once

#include "pcr/core/grid_config.h"
#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace pcr {
namespace detail {

// A refusal at create (InvalidArgument), as every plan routine words it.
inline Status refuse(const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: " + msg); }

// plane bits = PCR_HIP_PLANE_* of include/pcr_hip.h (sum, weight, max, min)
constexpr uint32_t kPlaneBits[4] = {1u, 2u, 4u, 8u};

// The first six have an implementation in the reference (src/ops/reduction_registry.cpp:173-184), and Pipeline::create
// refuses the others (src/engine/pipeline.cpp:229-233).  MostRecent the reference only declares (builtin_ops.h:106-124);
// this build implements it for the Point glyph (include/pcr_hip.h "MostRecent").  Median, Percentile, PriorityMerge and
// Custom stay refused.
inline bool registered(ReductionType t) {
    switch (t) {
        case ReductionType::Sum: case ReductionType::Max: case ReductionType::Min:
        case ReductionType::Average: case ReductionType::WeightedAverage: case ReductionType::Count:
        case ReductionType::MostRecent:
            return true;
        default:
            return false;
    }
}

// A selection ("keep the entry with the greatest key"), not an accumulation: a group of its own, keyed by its key channel too.
inline bool is_select(ReductionType t) { return t == ReductionType::MostRecent; }

// What Pipeline::create checks of every ReductionSpec, on every engine.
inline Status check_reduction_specs(const std::vector<ReductionSpec>& reductions) {
    for (const auto& r : reductions) {
        if (!registered(r.type)) return Status::error(StatusCode::InvalidArgument, "pipeline: unknown reduction type");
        if (is_select(r.type) && r.timestamp_channel.empty())
            return Status::error(StatusCode::InvalidArgument, "pipeline: MostRecent requires a timestamp_channel");
    }
    return Status::success();
}

// src/engine/pipeline.cpp:500-508
inline bool glyph_reduction_ok(ReductionType t) {
    return t == ReductionType::WeightedAverage || t == ReductionType::Average ||
           t == ReductionType::Sum || t == ReductionType::Count;
}

inline uint32_t planes_for(ReductionType t) {
    switch (t) {
        case ReductionType::Sum: return kPlaneBits[0];
        case ReductionType::Count: return kPlaneBits[1];
        case ReductionType::Max: return kPlaneBits[2];
        case ReductionType::Min: return kPlaneBits[3];
        // MostRecent: at the host-visible boundary its state is the reference's two float planes, value in slot 0 and
        // timestamp in slot 1 (pack_state<MostRecentOp>, builtin_ops.h:178-183), in a group no accumulation shares
        default: return kPlaneBits[0] | kPlaneBits[1];      // Average, WeightedAverage, MostRecent
    }
}

inline bool same_glyph(const GlyphSpec& a, const GlyphSpec& b) {
    if (a.type != b.type) return false;
    if (a.type == GlyphType::Point) return true;
    return a.direction_channel == b.direction_channel && a.default_direction == b.default_direction &&
           a.half_length_channel == b.half_length_channel && a.default_half_length == b.default_half_length &&
           a.sigma_x_channel == b.sigma_x_channel && a.default_sigma_x == b.default_sigma_x &&
           a.sigma_y_channel == b.sigma_y_channel && a.default_sigma_y == b.default_sigma_y &&
           a.rotation_channel == b.rotation_channel && a.default_rotation == b.default_rotation &&
           a.max_radius_cells == b.max_radius_cells;
}

// planes a reduction's reference state is made of, in the reference's field order
// (builtin_ops.h: Sum{sum}, Max{val}, Min{val}, Count{count}, Average{sum,count}, WeightedAverage{wsum,wgt})
inline int state_planes_of(ReductionType t, int out[2]) {
    switch (t) {
        case ReductionType::Sum: out[0] = 0; return 1;
        case ReductionType::Count: out[0] = 1; return 1;
        case ReductionType::Max: out[0] = 2; return 1;
        case ReductionType::Min: out[0] = 3; return 1;
        default: out[0] = 0; out[1] = 1; return 2;           // Average, WeightedAverage {sum, weight}; MostRecent {value, timestamp}
    }
}

// Identity of plane slot p of a group as the checkpoints see it (builtin_ops.h: identity()).  select: a MostRecent group,
// {NaN 0x7FC00000, -FLT_MAX}.
inline float plane_identity(bool select, int p) {
    if (select) {
        if (p == 1) return -3.402823466e+38f;
        const uint32_t bits = 0x7FC00000u;
        float f;
        std::memcpy(&f, &bits, sizeof f);
        return f;
    }
    return p == 2 ? -3.402823466e+38f : p == 3 ? 3.402823466e+38f : 0.0f;
}

// The MostRecent fold on the host (include/pcr_hip.h): ord() maps float bits monotonically onto unsigned integers,
// word(t, v) = ord(t + 0.0f) << 32 | ord(v); a cell's state is the maximum word of its accepted points, 0 when it has none.
inline uint32_t select_ord(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
inline uint32_t select_unord(uint32_t u) { return (u >> 31) ? (u ^ 0x80000000u) : ~u; }
inline bool select_accepts(float t) { return t > -3.402823466e+38f; }      // false for NaN (combine_timestamped vs the identity)
inline uint64_t select_word(float t, float v) {
    uint32_t tb, vb;
    std::memcpy(&tb, &t, 4);
    std::memcpy(&vb, &v, 4);
    if (tb == 0x80000000u) tb = 0u;                                          // t + 0.0f
    return ((uint64_t)select_ord(tb) << 32) | select_ord(vb);
}
inline uint64_t select_word_of_state(float v, float t) { return select_accepts(t) ? select_word(t, v) : 0u; }
inline void select_state_of_word(uint64_t w, float* v, float* t) {
    if (!w) { *v = plane_identity(true, 0); *t = plane_identity(true, 1); return; }
    const uint32_t vb = select_unord((uint32_t)w), tb = select_unord((uint32_t)(w >> 32));
    std::memcpy(v, &vb, 4);
    std::memcpy(t, &tb, 4);
}

inline std::string default_band_name(const ReductionSpec& r) {
    return r.output_band_name.empty() ? r.value_channel + "_" + std::to_string(static_cast<int>(r.type)) : r.output_band_name;
}

// "{channel}_p{round(q * 100)}": a percentile band of a histogram and a percentile column of a zonal table.
inline std::string percentile_name(const std::string& channel, float q) {
    return channel + "_p" + std::to_string(std::lround((double)q * 100.0));
}
// PipelineConfig::histograms: the name of entry h's j-th percentile band, percentile_name unless given.
inline std::string histogram_band_name(const HistogramConfig& h, size_t j) {
    if (j < h.band_names.size() && !h.band_names[j].empty()) return h.band_names[j];
    return percentile_name(h.value_channel, h.percentiles[j]);
}
// PipelineConfig::extremes: the name of an entry's band, "{value_channel}_low" / "{value_channel}_high" unless given.
inline std::string extremes_band_name(const ExtremesConfig& e) {
    if (!e.band_name.empty()) return e.band_name;
    return e.value_channel + (e.side == ExtremeSide::Highest ? "_high" : "_low");
}
// PipelineConfig::cell_stats: the name of band j of an entry, "{value_channel}_mean" / "_var" / "_std" unless given.
inline std::string cell_stats_band_name(const CellStatsConfig& c, size_t j) {
    if (j < c.band_names.size() && !c.band_names[j].empty()) return c.band_names[j];
    const CellStat p = j < c.products.size() ? c.products[j] : CellStat::StdDev;
    return c.value_channel + (p == CellStat::Mean ? "_mean" : p == CellStat::Variance ? "_var" : "_std");
}
// ReductionSpec::filter: equal means the same predicates in the same order, field by field.
inline bool same_predicate(const FilterPredicate& a, const FilterPredicate& b) {
    return a.channel_name == b.channel_name && a.op == b.op && a.value == b.value && a.value_set == b.value_set;
}
inline bool same_filter(const FilterSpec& a, const FilterSpec& b) {
    if (a.predicates.size() != b.predicates.size()) return false;
    for (size_t k = 0; k < a.predicates.size(); ++k)
        if (!same_predicate(a.predicates[k], b.predicates[k])) return false;
    return true;
}
// The grouping key: ReductionSpecs that read the same value channel through the same glyph share one pass over the points and
// one set of planes.  A MostRecent spec is keyed by its timestamp channel too and never shares a group with the accumulations;
// specs with different filters see different points and never share a group either.
inline bool same_group(const ReductionSpec& a, const ReductionSpec& b) {
    if (is_select(a.type) != is_select(b.type)) return false;
    if (is_select(a.type) && a.timestamp_channel != b.timestamp_channel) return false;
    return a.value_channel == b.value_channel && same_glyph(a.glyph, b.glyph) && same_filter(a.filter, b.filter);
}

// ---- the grouping plan: a configuration's accumulation groups and outputs, the same on every engine ------------------------
struct GroupSpec {                       // one pass over the points, one set of planes
    std::string value_channel;
    GlyphSpec glyph;
    bool select = false;                 // a MostRecent group (plane slots 0 / 1 = value / timestamp)
    std::string key_channel;             // ... and its timestamp channel
    FilterSpec filter;                   // ReductionSpec::filter of the group's specs
    int cls = 0;                         // its filter class (FilterPlan): 0 = PipelineConfig::filter alone
    uint32_t mask = 0;                   // kPlaneBits of the planes it keeps
};
struct Output {                          // one band finalize makes from the state: a ReductionSpec's, a percentile band or an
                                         // extremes band
    int group = 0;                       // -1: a percentile band of histogram `hist` (no group reads or writes it; its type is
                                         // Max, so that it is filled like a Max band), or the band of extremes entry `ext` (its
                                         // type is Min for Lowest, Max for Highest, for the same reason)
    ReductionType type = ReductionType::Sum;
    std::string band_name;
    int hist = -1, q = 0;                // the histogram and which of its percentiles
    int ext = -1;                        // the extremes entry
    int stat = -1, product = 0;          // the cell-stats entry and which of its products (group -1 too; the type is Average for
                                         // a Mean band, filled like an Average band, and Sum for Variance and StdDev, which
                                         // fills_nodata rejects: a spread is never filled.  The type of a group -1 output decides
                                         // nothing but that)
};
struct GroupPlan {
    std::vector<GroupSpec> groups;       // in order of first appearance among the ReductionSpecs: reduction_groups(), state_planes(),
                                         // parked windows (planes[4 g + p]) and the `.pcrt` directories all count them this way
    std::vector<Output> outputs;         // the result grid's order: one per ReductionSpec, then the histograms' percentile bands entry
                                         // by entry, then one band per extremes entry, then the cell-stats bands entry by entry.
                                         // What ground.source_band, ground.top_band and terrain[].source_band may name (the DTM,
                                         // hag and terrain bands follow them)
};
GroupPlan plan_groups(const PipelineConfig& cfg);
// The outputs a checkpoint carries (write_state_tiles, read_state_tiles): those with a group.
inline std::vector<Output> state_outputs(const std::vector<Output>& outputs) {
    std::vector<Output> o;
    for (const auto& out : outputs)
        if (out.group >= 0) o.push_back(out);
    return o;
}
inline std::vector<std::string> output_band_names(const PipelineConfig& cfg) {
    std::vector<std::string> names;
    for (const auto& o : plan_groups(cfg).outputs) names.push_back(o.band_name);
    return names;
}

// Host copies of state planes over the row WINDOW [row0, row0 + rows) of the grid (whole tile rows for everything below):
// plane(group, p) -> rows x width floats, or null when the group has no plane p.
struct StateWindow {
    int row0 = 0, rows = 0;
    int own_row0 = -1, own_row1 = -1;      // >= 0: only tiles whose rows lie inside [own_row0, own_row1) (a shard with apron rows)
    std::function<float*(int group, int p)> plane;
};
/// The window [row0, row0 + rows) over host copies laid out planes[4 g + p] (empty: group g has no plane p).
inline StateWindow window_over(std::vector<std::vector<float>>& planes, int row0, int rows) {
    StateWindow w;
    w.row0 = row0;
    w.rows = rows;
    w.plane = [&planes](int g, int p) -> float* {
        auto& v = planes[(size_t)g * 4 + (size_t)p];
        return v.empty() ? nullptr : v.data();
    };
    return w;
}

/// The C-ABI's view of a whole grid: own and state rows cover the full height (a shard overrides its rows and halo).
inline pcr_hip_grid to_hip_grid(const GridConfig& g) {
    pcr_hip_grid hg{};
    hg.min_x = g.bounds.min_x; hg.min_y = g.bounds.min_y; hg.max_x = g.bounds.max_x; hg.max_y = g.bounds.max_y;
    hg.cell_size_x = g.cell_size_x; hg.cell_size_y = g.cell_size_y;
    hg.width = g.width; hg.height = g.height;
    hg.tile_width = g.tile_width; hg.tile_height = g.tile_height;
    hg.own_row0 = 0; hg.own_row1 = g.height;
    hg.state_row0 = 0; hg.state_rows = g.height;
    return hg;
}

// ---- the filter stage, planned at create on every engine --------------------------------------------------------------------
// Class 0 is PipelineConfig::filter alone (the specs with an empty filter); class k >= 1 is the k-th distinct non-empty spec
// filter in order of first appearance.  A point contributes to a spec when it passes PipelineConfig::filter AND the spec's
// class: words[k] is that conjunction as bits of `table`, the distinct predicates of the whole configuration.
constexpr size_t kMaxSpecFilters = 8;
struct FilterPlan {
    std::vector<FilterSpec> classes;         // [0] is empty
    std::vector<int> class_of;               // per ReductionSpec
    std::vector<int> hist_class_of;          // per entry of PipelineConfig::histograms: its filter joins the same plan
    std::vector<int> ext_class_of;           // per entry of PipelineConfig::extremes: likewise
    std::vector<int> stat_class_of;          // per entry of PipelineConfig::cell_stats: likewise
    std::vector<std::vector<int>> pz_stat_class_of, pz_hist_class_of;   // per entry of PipelineConfig::point_zonal, per spec: likewise
    std::vector<FilterPredicate> table;      // PipelineConfig::filter's predicates first
    std::vector<uint32_t> words;             // per class; words[0] == 0: no PipelineConfig::filter
    bool any() const { return classes.size() > 1; }
};
/// InvalidArgument, with the same message on every engine, for more than kMaxSpecFilters distinct non-empty spec filters, a
/// conjunction longer than PCR_HIP_MAX_FILTER_PREDICATES, or more than PCR_HIP_MAX_CLASS_PREDICATES distinct predicates.  A
/// configuration without spec filters is refused nothing: a PipelineConfig::filter of more distinct predicates than the table
/// holds gets no table and no words (the host engine reads `classes` alone; validate_cloud refuses it on the device, at ingest).
Status plan_filters(const PipelineConfig& cfg, FilterPlan* out);

// ---- the filter stage on the device (pcr_hip_filter_classes) ---------------------------------------------------------------
/// Device pointer of a named Float32 channel of the cloud being ingested (null: the cloud has no such channel).
using ChannelLookup = std::function<Status(const std::string& name, const float** d_channel)>;
/// The FilterSpec as the C-ABI takes it, its channels resolved through `channel` in the predicates' order.
Status marshal_predicates(const FilterSpec& filter, const ChannelLookup& channel, std::vector<pcr_hip_predicate>* out);
/// Device memory the stage needs for n points, laid out [128 B: u64 survivor counts][class masks, each a multiple of 16 bytes
/// apart; no mask for class 0 without a PipelineConfig::filter].  0: the plan filters nothing.
size_t filter_stage_bytes(const FilterPlan& plan, size_t n);
/// ONE sweep over the points (pcr_hip_filter_classes; eight classes per call, so nine masks take a second one) makes the mask of
/// every class of the plan in d_buffer.  (*masks)[k]: class k's mask; null for class 0 when there is no PipelineConfig::filter
/// (every point is kept).  *kept: PipelineConfig::filter's survivors, read back with one host wait -- only when there is such a
/// filter; without one the sweep is enqueued and nothing waited for.  A plan that filters nothing launches nothing.
Status sweep_filter_classes(const FilterPlan& plan, const ChannelLookup& channel, size_t n, void* d_buffer, pcr_hip_stream stream,
                            std::vector<const uint8_t*>* masks, size_t* kept);

// ---- reprojection on ingest (PipelineConfig::target_crs / auto_reproject; pcr/core/reproject.h) ---------------------------
/// CRS -> the C-ABI's descriptor; CrsError when it is unidentified or not supported.  role: "source" / "destination".
Status crs_desc(const CRS& crs, const char* role, pcr_hip_crs_desc* out);
/// pcr_hip_transform_xy_host over `threads` OpenMP threads, in chunks.
Status transform_host(const pcr_hip_crs_desc& src, const pcr_hip_crs_desc& dst, const double* x, const double* y, double* ox,
                      double* oy, size_t n, int threads);
/// What an ingest does about the cloud's CRS, decided before any state changes.  The destination is the grid's CRS when it
/// is valid, else target_crs.  The cloud is reprojected only when auto_reproject is set, both CRSs are identified
/// (crs_epsg) and their codes differ; anything else -- unidentified, untagged, equal -- ingests the coordinates as they are.
struct Reprojection {
    bool needed = false;
    pcr_hip_crs_desc src{}, dst{};
    CRS dst_crs;                         // what the reprojected points are tagged with
};
/// CrsError (naming both codes; nothing may be accumulated then) when both are identified and differ but either is not
/// supported.
Status plan_reprojection(const PipelineConfig& cfg, const PointCloud& cloud, Reprojection* out);

/// "<dir>" for a single reduction (the reference's layout), "<dir>/reduction_<r>" otherwise.
std::string reduction_state_dir(const std::string& dir, size_t r, size_t n_outputs);

// What every engine checks of a cloud before it touches any state, with the reference's messages: the filter's channels
// (filter_points, src/engine/filter.cpp:101-123), every reduction's value channel and glyph / reduction pairing
// (src/engine/pipeline.cpp:365-378, 500-508).  max_set / max_predicates: the device filter's limits (0 = none, host engine).
Status validate_cloud(const PipelineConfig& cfg, const PointCloud& cloud, size_t max_set, size_t max_predicates);
/// One `.pcrt` file per touched reference tile inside the window and per output (src/io/tile_state_io.cpp:45-95;
/// file name src/io/tile_state_io.cpp:197-211).  touched: tiles_x * tiles_y flags of the whole grid.
Status write_state_tiles(const GridConfig& g, const std::vector<Output>& outputs, const StateWindow& w,
                         const std::vector<uint32_t>& touched, const std::string& dir, std::vector<std::string>* written = nullptr);
/// The reverse: every matching file inside the window is copied into the planes and its tile marked touched; files that do
/// not describe their tile of their reduction are ignored like the reference's tile manager ignores them
/// (src/engine/tile_manager.cpp:272-320).  *loaded = files taken.
Status read_state_tiles(const GridConfig& g, const std::vector<Output>& outputs, const StateWindow& w,
                        std::vector<uint32_t>& touched, const std::string& dir, size_t* loaded);

}  // namespace detail
}  // namespace pcr
