// host_pipeline.cpp -- see host_pipeline.h.
#include "host_pipeline.h"

#include "fill_nodata.h"
#include "ground_filter.h"
#include "polygonize.h"
#include "terrain.h"
#include "trees.h"
#include "pcr/core/point_cloud.h"
#include "pcr/io/grid_io.h"

#include <algorithm>
#include <map>

namespace pcr {

Status Pipeline::Host::init() {
    const GridConfig& g = cfg.grid;
    if (g.width <= 0 || g.height <= 0)
        return Status::error(StatusCode::InvalidArgument, "pipeline: grid dimensions must be positive");
    if (g.tile_width <= 0 || g.tile_height <= 0)
        return Status::error(StatusCode::InvalidArgument, "pipeline: tile dimensions must be positive");
    {
        Status ok = detail::check_reduction_specs(cfg.reductions);
        if (ok.ok()) ok = detail::check_histograms(cfg);
        if (ok.ok()) ok = detail::check_extremes(cfg);
        if (ok.ok()) ok = detail::check_cell_stats(cfg);
        if (ok.ok()) ok = detail::plan_filters(cfg, &filters);
        if (ok.ok()) ok = detail::plan_point_zonal(cfg, filters, &pz_plan);
        if (ok.ok()) ok = pz_state.allocate(pz_plan, MemoryLocation::Host, nullptr);
        if (!ok.ok()) return ok;
    }
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0)
        return Status::error(StatusCode::InvalidArgument, "pipeline: row-block shards run on the GPU engine only (one process per GPU)");
    if (cfg.result_location == MemoryLocation::Device)
        return Status::error(StatusCode::InvalidArgument, "pipeline: the CPU engine's result lives in host memory (result_location = Device asked)");
    {
        Status ok = detail::plan_surfaces(cfg);
        if (!ok.ok()) return ok;
        surfaces.resize(cfg.surface_channels.size());
        if (!(ok = detail::plan_polygon_channels(cfg)).ok()) return ok;
        polygon_sets.resize(cfg.polygon_channels.size());
    }
    engine = std::make_unique<detail::HostEngine>(g, (int)cfg.cpu_threads);        // cpu_threads = 0: every core (pipeline.h:78)
    {
        detail::GroupPlan plan = detail::plan_groups(cfg);
        groups.resize(plan.groups.size());
        for (size_t gi = 0; gi < groups.size(); ++gi) static_cast<detail::GroupSpec&>(groups[gi]) = plan.groups[gi];
        outputs = std::move(plan.outputs);
    }
    // PipelineConfig::histograms: the cubes
    hist = detail::plan_histograms(cfg, filters);
    for (size_t h = 0; h < hist.entries.size(); ++h) cubes.emplace_back(hist.entries[h].cube_cells((size_t)g.width * g.height), 0u);
    // PipelineConfig::extremes: the key planes, all EMPTY
    ext = detail::plan_extremes(cfg, filters);
    for (const auto& e : ext.entries) ext_keys.emplace_back(e.state_cells((size_t)g.width * g.height), 0xFFFFFFFFu);
    // PipelineConfig::cell_stats: the three planes, zero
    cstats = detail::plan_cell_stats(cfg, filters);
    stat_planes.resize(cstats.entries.size());
    for (auto& p : stat_planes) {
        p.n.assign((size_t)g.width * g.height, 0u);
        p.s1.assign((size_t)g.width * g.height, 0);
        p.s2.assign((size_t)g.width * g.height, 0u);
    }
    // Tile state is identity-initialised (src/engine/tile_manager.cpp:183-260); here for the whole grid at once.
    for (auto& gr : groups) engine->init_planes(gr.planes, gr.mask, gr.select);
    if (!cfg.zonal.empty()) {                                        // PipelineConfig::zonal: only the plan
        detail::GroundPlan ground;
        detail::TerrainPlan terrain;
        detail::TreesPlan trees;
        Status ok = detail::plan_ground(cfg, &ground);
        if (ok.ok()) ok = detail::plan_terrain(cfg, ground, &terrain);
        if (ok.ok()) ok = detail::plan_trees(cfg, ground, terrain, &trees);
        if (ok.ok()) ok = detail::plan_zonal(cfg, ground, terrain, trees, &zonal_plan);
        if (!ok.ok()) return ok;
    }
    return Status::success();
}

// PipelineConfig::zonal: the label band of an external entry into host memory the pipeline owns.
Status Pipeline::Host::set_zones(const std::string& name, const Grid& grid, int band) {
    return detail::store_zones(cfg, name, grid, band, MemoryLocation::Host, nullptr, &zone_grids);
}
Status Pipeline::Host::set_zones(const std::string& name, const PolygonSet& polygons, const RasterizeOptions& options) {
    return detail::store_zones(cfg, name, polygons, options, MemoryLocation::Host, nullptr, &zone_grids);
}
// The table of entry i through the C-ABI's host twins: the label band of the result, the planes and the cubes where they are.
Status Pipeline::Host::zonal(int i, ZonalTable* out, bool with_counts) const {
    if (!out || i < 0 || !finalized || !zonal_fresh || !result || (size_t)i >= zonal_plan.entries.size())
        return Status::error(StatusCode::InvalidArgument,
                             "pipeline: zonal: no zonal entry " + std::to_string(i) + " (of a finalize with no ingest since)");
    const auto& e = zonal_plan.entries[(size_t)i];
    detail::ZonalInputs in;
    in.width = cfg.grid.width;
    in.rows = cfg.grid.height;
    if (e.band >= 0) {
        in.zones = result->band_f32(e.band);
    } else {
        const auto it = zone_grids.find(e.zones);
        if (it == zone_grids.end())
            return Status::error(StatusCode::InvalidArgument, "pipeline: zonal: the label grid '" + e.zones + "' was not set (set_zones)");
        in.zones = static_cast<const float*>(it->second.band.data());
    }
    for (const auto& p : stat_planes)
        in.stats.push_back({p.n.data(), reinterpret_cast<const long long*>(p.s1.data()), reinterpret_cast<const unsigned long long*>(p.s2.data())});
    for (const auto& c : cubes) in.cubes.push_back(c.data());
    return detail::zonal_table(e, cstats, hist, in, with_counts, out);
}

// The zones of a band of the result as polygons, by the host twin.
Status Pipeline::Host::polygonize(const std::string& band_name, PolygonSet* out) const {
    int b = -1;
    if (Status s = detail::polygonize_check(cfg, out, finalized && zonal_fresh, result.get(), band_name, &b); !s.ok()) return s;
    return detail::polygonize_band(result->band_f32(b), cfg.grid, MemoryLocation::Host, nullptr, out);
}

// PipelineConfig::point_zonal: entry i's rows through the C-ABI's host twins, from the tables as the ingests left them.
Status Pipeline::Host::point_zonal(int i, PointZonalTable* out, bool with_counts) const {
    if (!out || i < 0 || (size_t)i >= pz_plan.entries.size())
        return Status::error(StatusCode::InvalidArgument, "pipeline: point_zonal: no point_zonal entry " + std::to_string(i));
    return detail::point_zonal_table(pz_plan.entries[(size_t)i], pz_state.tables[(size_t)i], nullptr, with_counts, out);
}

// PipelineConfig::surface_channels: the band and its geometry into host memory the pipeline owns.
Status Pipeline::Host::set_surface(const std::string& name, const Grid& grid, int band) {
    int index = -1;
    pcr_hip_grid geom{};
    Status s = detail::check_surface(cfg, name, grid, band, &index, &geom);
    return s.ok() ? detail::store_surface(grid, band, geom, MemoryLocation::Host, nullptr, &surfaces[(size_t)index]) : s;
}

// PipelineConfig::polygon_channels: the index, built and kept on the host.
Status Pipeline::Host::set_polygons(const std::string& name, const PolygonSet& polygons, const PointInPolygonOptions& options) {
    return detail::store_polygons(cfg, name, polygons, options, false, nullptr, &polygon_sets);
}

Status Pipeline::Host::ingest(const PointCloud& cloud_in) {
    const size_t n = cloud_in.count();
    if (n == 0) return Status::success();                            // pipeline.cpp:284-287
    std::unique_ptr<PointCloud> copy;
    const PointCloud* cloud = &cloud_in;
    if (cloud->location() == MemoryLocation::Device) {
        copy = cloud->to(MemoryLocation::Host);
        if (!copy) return Status::error(StatusCode::OutOfMemory, "pipeline: cannot copy the device cloud to the host");
        cloud = copy.get();
    }
    // the reference's checks and messages (pipeline_common.cpp; no device limits on the host)
    if (!surfaces.empty()) {
        Status ok = detail::validate_surfaces(cfg, *cloud, surfaces);
        if (!ok.ok()) return ok;
    }
    if (!polygon_sets.empty()) {
        Status ok = detail::validate_polygon_channels(cfg, *cloud, polygon_sets);
        if (!ok.ok()) return ok;
    }
    {
        Status ok = detail::validate_cloud(cfg, *cloud, 0, 0);
        if (ok.ok() && pz_plan.on()) ok = detail::validate_point_zonal(cfg, *cloud);
        if (!ok.ok()) return ok;
    }
    // a cloud in another CRS than the grid's: its coordinates transformed into host vectors (the cloud stays as it is)
    detail::Reprojection rp;
    {
        Status ok = detail::plan_reprojection(cfg, *cloud, &rp);
        if (!ok.ok()) return ok;
    }
    std::vector<double> rx, ry;
    const double* px = cloud->x();
    const double* py = cloud->y();
    if (rp.needed) {
        rx.resize(n);
        ry.resize(n);
        Status ok = detail::transform_host(rp.src, rp.dst, px, py, rx.data(), ry.data(), n, engine->threads());
        if (!ok.ok()) return ok;
        px = rx.data();
        py = ry.data();
    }
    // Surface channels: each gathered once, for all n points, at the (reprojected) coordinates -- the host loop of the C-ABI, so
    // the bits are the HIP engine's -- and then found by name like a channel the cloud brought.
    std::map<std::string, std::vector<float>> derived;
    for (size_t k = 0; k < surfaces.size(); ++k) {
        const SurfaceChannelConfig& sc = cfg.surface_channels[k];
        std::vector<float>& out = derived[sc.name];
        out.resize(n);
        const detail::Surface& sf = surfaces[k];
        Status ok = detail::sample_host(sf.geom, static_cast<const float*>(sf.band.data()), sf.geom.width, px, py,
                                        sc.value_channel.empty() ? nullptr : cloud->channel_f32(sc.value_channel), n, sc.mode,
                                        out.data(), engine->threads());
        if (!ok.ok()) return ok;
    }
    // Polygon channels, beside them: the host twin of the C-ABI at the same coordinates, so the bits are the HIP engine's.
    for (size_t k = 0; k < polygon_sets.size(); ++k) {
        std::vector<float>& out = derived[cfg.polygon_channels[k].name];
        out.resize(n);
        Status ok = polygon_sets[k]->locate(px, py, n, out.data(), false, nullptr, engine->threads());
        if (!ok.ok()) return ok;
    }
    auto f32 = [&](const std::string& name) -> const float* {
        if (name.empty()) return nullptr;
        const auto hit = derived.find(name);
        if (hit != derived.end()) return hit->second.data();
        const ChannelDesc* d = cloud->channel(name);
        if (!d || d->dtype != DataType::Float32) return nullptr;     // -> GlyphSpec default
        return cloud->channel_f32(name);
    };

    // Filter stage: AND of the predicates (evaluate_predicate, src/engine/filter.cpp:34-56).  As in the HIP pipeline a
    // filtered-out point does not exist for any reduction (the reference routes the unfiltered cloud: DESIGN section 1).
    // ReductionSpec::filter: `keep` (cfg.filter) routes the cloud and sets the touched flags; a group with a filter of its own
    // folds only the points its class keeps on top of that (class_keep[k], the spec filter alone: a point cfg.filter drops is
    // routed nowhere).  Byte masks, so the bits are the same at any thread count.
    auto apply = [&](const FilterSpec& filter, std::vector<uint8_t>& keep) {
        keep.assign(n, 1);
        for (const auto& pr : filter.predicates) {
            const float* ch = f32(pr.channel_name);
            const int team = engine->threads();
#pragma omp parallel for num_threads(team) schedule(static)
            for (int64_t i = 0; i < (int64_t)n; ++i) {
                const float v = ch[i];
                bool ok = false;
                switch (pr.op) {
                    case CompareOp::Equal: ok = v == pr.value; break;
                    case CompareOp::NotEqual: ok = v != pr.value; break;
                    case CompareOp::Less: ok = v < pr.value; break;
                    case CompareOp::LessEqual: ok = v <= pr.value; break;
                    case CompareOp::Greater: ok = v > pr.value; break;
                    case CompareOp::GreaterEqual: ok = v >= pr.value; break;
                    case CompareOp::InSet:
                    case CompareOp::NotInSet: {
                        bool in = false;
                        for (float sv : pr.value_set) in = in || v == sv;
                        ok = pr.op == CompareOp::InSet ? in : !in;
                        break;
                    }
                }
                if (!ok) keep[(size_t)i] = 0;
            }
        }
    };
    std::vector<uint8_t> keep;
    size_t kept = n;
    if (!cfg.filter.empty()) {
        apply(cfg.filter, keep);
        kept = 0;
        for (uint8_t k : keep) kept += k;
        if (kept == 0) return Status::success();                     // pipeline.cpp:349-353
    }
    // (this cloud's points change the state: a cloud that is empty or that PipelineConfig::filter empties changes nothing, and the
    // tables of the last finalize stay valid -- as on the HIP engine)
    zonal_fresh = false;
    std::vector<std::vector<uint8_t>> class_keep(filters.classes.size());
    for (size_t k = 1; k < filters.classes.size(); ++k) apply(filters.classes[k], class_keep[k]);
    auto keep_of = [&](const Group& gr, size_t i0) -> const uint8_t* { return gr.cls ? class_keep[(size_t)gr.cls].data() + i0 : nullptr; };
    auto hist_keep = [&](const detail::HistogramEntry& e, size_t i0) -> const uint8_t* { return e.cls ? class_keep[(size_t)e.cls].data() + i0 : nullptr; };
    auto ext_keep = [&](const detail::ExtremesEntry& e, size_t i0) -> const uint8_t* { return e.cls ? class_keep[(size_t)e.cls].data() + i0 : nullptr; };
    auto stat_keep = [&](const detail::CellStatsEntry& e, size_t i0) -> const uint8_t* { return e.cls ? class_keep[(size_t)e.cls].data() + i0 : nullptr; };

    // the engine indexes a cloud with 32 bits: larger ones go in slices
    const size_t slice = (size_t)1 << 31;
    size_t valid = 0;
    for (size_t i0 = 0; i0 < n; i0 += slice) {
        const size_t m = std::min(slice, n - i0);
        valid += engine->route(px + i0, py + i0, keep.empty() ? nullptr : keep.data() + i0, m);
        for (auto& gr : groups) {
            const float* v = f32(gr.value_channel);
            if (gr.select) {                                         // (Point glyph: validate_cloud refused anything else)
                engine->scatter_select(gr.planes, v + i0, f32(gr.key_channel) + i0, keep_of(gr, i0));
            } else if (gr.glyph.type == GlyphType::Point) {
                engine->scatter_point(gr.planes, v + i0, keep_of(gr, i0));
            } else {
                detail::HostGlyphArrays arr;
                auto at = [&](const std::string& name) { const float* p = f32(name); return p ? p + i0 : nullptr; };
                arr.direction = at(gr.glyph.direction_channel);
                arr.half_length = at(gr.glyph.half_length_channel);
                arr.sigma_x = at(gr.glyph.sigma_x_channel);
                arr.sigma_y = at(gr.glyph.sigma_y_channel);
                arr.rotation = at(gr.glyph.rotation_channel);
                detail::HostPlanes& pl = gr.planes;
                const uint32_t keep_mask = pl.mask;
                pl.mask &= 3u;                                        // glyph reductions feed the sum and weight planes only
                engine->scatter_glyph(pl, gr.glyph, arr, v + i0, keep_of(gr, i0));
                pl.mask = keep_mask;
            }
        }
        for (size_t h = 0; h < hist.entries.size(); ++h) {
            const detail::HistogramEntry& e = hist.entries[h];
            engine->scatter_histogram(cubes[h].data(), e.bins, e.lo, e.inv_w, f32(e.value_channel) + i0, hist_keep(e, i0));
        }
        for (size_t x = 0; x < ext.entries.size(); ++x) {
            const detail::ExtremesEntry& e = ext.entries[x];
            engine->scatter_extremes(ext_keys[x].data(), e.k, e.side, f32(e.value_channel) + i0, ext_keep(e, i0));
        }
        for (size_t x = 0; x < cstats.entries.size(); ++x) {
            const detail::CellStatsEntry& e = cstats.entries[x];
            StatPlanes& p = stat_planes[x];
            engine->scatter_cell_stats(p.n.data(), p.s1.data(), p.s2.data(), e.origin, e.inv_res, f32(e.value_channel) + i0, stat_keep(e, i0));
        }
    }
    if (pz_plan.on()) {
        // PipelineConfig::point_zonal: the twins on the same masks as the device's classes -- PipelineConfig::filter AND the class's
        // own, made once per class that an entry uses.  The grid plays no part: all n points, routed or not.
        std::vector<std::vector<uint8_t>> both(filters.classes.size());
        detail::PointZonalInputs in;
        in.n = n;
        in.channel = [&](const std::string& name, const float** p) { *p = f32(name); return Status::success(); };
        in.mask = [&](int cls) -> const uint8_t* {
            if (cls == 0) return keep.empty() ? nullptr : keep.data();
            if (keep.empty()) return class_keep[(size_t)cls].data();
            std::vector<uint8_t>& m = both[(size_t)cls];
            if (m.empty()) {
                m.resize(n);
                for (size_t i = 0; i < n; ++i) m[i] = keep[i] & class_keep[(size_t)cls][i];
            }
            return m.data();
        };
        Status ok = detail::point_zonal_fold(pz_plan, pz_state, in);
        if (!ok.ok()) return ok;
    }
    last = ScatterInfo{};
    last.path = -1;                                                  // neither of the device's scatter paths
    last.points_in = n;
    last.points_valid = valid;
    points += kept;                                                  // points_processed += filtered_count (pipeline.cpp:749)
    collections++;
    if (callback) {
        ProgressInfo info = stats();
        if (!callback(info)) return Status::error(StatusCode::InvalidArgument, "pipeline: cancelled by user");
    }
    return Status::success();
}

Status Pipeline::Host::finalize() {
    if (outputs.empty()) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate result grid");
    const GridConfig& g = cfg.grid;
    detail::GroundPlan ground;
    Status gs = detail::plan_ground(cfg, &ground);
    if (!gs.ok()) return gs;
    detail::TerrainPlan terrain;
    if (!(gs = detail::plan_terrain(cfg, ground, &terrain)).ok()) return gs;
    detail::TreesPlan trees;
    if (!(gs = detail::plan_trees(cfg, ground, terrain, &trees)).ok()) return gs;
    if (!result) {
        std::vector<BandDesc> bands;
        for (const auto& o : outputs) {                              // band naming: pipeline.cpp:1175-1186
            BandDesc b;
            b.name = o.band_name;
            b.dtype = DataType::Float32;
            b.is_state = false;
            bands.push_back(b);
        }
        detail::append_ground_bands(ground, bands);
        detail::append_terrain_bands(terrain, bands);
        detail::append_tree_bands(trees, bands);
        result = Grid::create(g.width, g.height, bands, MemoryLocation::Host);
        if (!result) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate result grid");
        (void)result->set_geometry(detail::result_geometry(cfg));
    }
    for (size_t r = 0; r < outputs.size(); ++r)
        if (outputs[r].group >= 0) engine->finalize(groups[(size_t)outputs[r].group].planes, outputs[r].type, result->band_f32((int)r));
    for (size_t h = 0, r = cfg.reductions.size(); h < hist.entries.size(); r += hist.entries[h].q.size(), ++h) {
        // (one walk per histogram: its bands are consecutive outputs)
        std::vector<float*> dsts;
        for (size_t j = 0; j < hist.entries[h].q.size(); ++j) dsts.push_back(result->band_f32((int)(r + j)));
        Status hs = detail::percentiles_host(hist.entries[h], cubes[h].data(), g.width, g.height, dsts.data(), engine->threads());
        if (!hs.ok()) return hs;
    }
    for (size_t x = 0, r = cfg.reductions.size() + (size_t)hist.extra_bands(); x < ext.entries.size(); ++x, ++r) {
        Status es = detail::extremes_band_host(ext.entries[x], ext_keys[x].data(), g.width, g.height, result->band_f32((int)r), nullptr,
                                               engine->threads());
        if (!es.ok()) return es;
    }
    for (size_t x = 0, r = cfg.reductions.size() + (size_t)hist.extra_bands() + (size_t)ext.extra_bands(); x < cstats.entries.size(); ++x) {
        const detail::CellStatsEntry& e = cstats.entries[x];
        std::vector<float*> dsts;
        for (size_t j = 0; j < e.products.size(); ++j) dsts.push_back(result->band_f32((int)(r + j)));
        Status cs = detail::cell_stats_bands_host(e, stat_planes[x].n.data(), stat_planes[x].s1.data(), stat_planes[x].s2.data(), g.width,
                                                  g.height, dsts.data(), engine->threads());
        if (!cs.ok()) return cs;
        r += e.products.size();
    }
    {                                                                // (the planes are the state: the bands are made anew by every finalize)
        std::vector<ReductionType> types;
        for (const auto& o : outputs) types.push_back(o.type);
        Status fs = detail::finish_result_host(*result, types, cfg.fill_nodata_radius, ground, terrain, trees, &tree_tables, &tree_status);
        if (!fs.ok()) return fs;
    }
    finalized = true;
    zonal_fresh = true;
    if (!cfg.output_path.empty()) return write_geotiff(cfg.output_path, *result, g, pipeline_output_options(cfg.write_cog));    // pipeline.cpp:1351-1361
    return Status::success();
}

Status Pipeline::Host::save_state(const std::string& dir_in) {
    if (!cfg.histograms.empty()) return detail::histograms_checkpoint_error();
    if (!cfg.extremes.empty()) return detail::extremes_checkpoint_error();
    if (!cfg.cell_stats.empty()) return detail::cell_stats_checkpoint_error();
    if (!cfg.point_zonal.empty()) return detail::point_zonal_checkpoint_error();
    const std::string dir = dir_in.empty() ? cfg.state_dir : dir_in;
    if (dir.empty()) return Status::error(StatusCode::InvalidArgument, "pipeline: no state directory given");
    detail::StateWindow w;
    w.row0 = 0;
    w.rows = cfg.grid.height;
    w.plane = [&](int g, int p) -> float* { auto& v = groups[(size_t)g].planes.plane[p]; return v.empty() ? nullptr : v.data(); };
    return detail::write_state_tiles(cfg.grid, detail::state_outputs(outputs), w, engine->touched(), dir);
}

Status Pipeline::Host::load_state(const std::string& dir_in) {
    if (!cfg.histograms.empty()) return detail::histograms_checkpoint_error();
    if (!cfg.extremes.empty()) return detail::extremes_checkpoint_error();
    if (!cfg.cell_stats.empty()) return detail::cell_stats_checkpoint_error();
    if (!cfg.point_zonal.empty()) return detail::point_zonal_checkpoint_error();
    const std::string dir = dir_in.empty() ? cfg.state_dir : dir_in;
    if (dir.empty()) return Status::error(StatusCode::InvalidArgument, "pipeline: no state directory given");
    detail::StateWindow w;
    w.row0 = 0;
    w.rows = cfg.grid.height;
    w.plane = [&](int g, int p) -> float* { auto& v = groups[(size_t)g].planes.plane[p]; return v.empty() ? nullptr : v.data(); };
    Status s = detail::read_state_tiles(cfg.grid, detail::state_outputs(outputs), w, engine->touched(), dir, nullptr);
    for (auto& gr : groups) engine->normalize_select(gr.planes);     // a state read from a file is judged by the acceptance rule again
    return s;
}

ProgressInfo Pipeline::Host::stats() const {
    ProgressInfo info;
    info.collections_processed = collections;
    info.collections_total = 0;
    info.points_processed = points;
    info.tiles_active = engine ? engine->tiles_active() : 0;
    info.elapsed_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
    return info;
}

}  // namespace pcr
