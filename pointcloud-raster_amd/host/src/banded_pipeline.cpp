// banded_pipeline.cpp -- Pipeline::Banded (banded_pipeline.h): band planning at create, the visits of ingest and finalize,
// the host cache with its `.pcrt` spill, checkpoints of the whole pipeline.
#include "banded_pipeline.h"
#include "sample_grid.h"

#include "buffer.h"
#include "device_pipeline.h"
#include "fill_nodata.h"
#include "ground_filter.h"
#include "terrain.h"
#include "trees.h"
#include "pcr/core/point_cloud.h"
#include "pcr/io/grid_io.h"

#include <algorithm>
#include <cstdio>
#include <filesystem>
#include <limits>

#include <unistd.h>

namespace pcr {

using detail::kPlaneBits;

bool Pipeline::Banded::needed(const PipelineConfig& config, size_t* budget) {
    const GridConfig& g = config.grid;
    if (!(config.shard_row_begin < 0 && config.shard_row_end < 0 && config.exec_mode != ExecutionMode::CPU && g.width > 0 && g.height > 0 &&
          g.tile_height > 0 && !config.reductions.empty() && cuda_device_available() && config.cuda_device_id >= 0 &&
          config.cuda_device_id < cuda_device_count())) return false;
    *budget = config.gpu_memory_budget;
    if (*budget == 0) {
        size_t free_mem = 0, total_mem = 0;
        if (cuda_get_memory_info(&free_mem, &total_mem, config.cuda_device_id)) *budget = (size_t)(free_mem * 0.8);
    }
    // (PipelineConfig::point_zonal: its tables are state in HBM too, whatever the grid's size)
    return *budget > 0 && bytes_per_row(config) * (size_t)g.height + detail::point_zonal_state_bytes(config) > *budget;
}

std::unique_ptr<Pipeline::Banded> Pipeline::Banded::create(const PipelineConfig& config, const Pipeline* owner, size_t budget, Status* st) {
    const GridConfig& g = config.grid;
    const size_t per_row = bytes_per_row(config);
    if (!(*st = detail::check_reduction_specs(config.reductions)).ok()) return nullptr;
    detail::FilterPlan filters;                       // (the bands' sub-pipelines plan again: here the refusals and any())
    if (!(*st = detail::plan_filters(config, &filters)).ok()) return nullptr;
    const int th = g.tile_height;
    const size_t fit = budget / std::max<size_t>(per_row * (size_t)th, 1);          // whole tile rows that fit
    const int band_rows = (int)std::min<size_t>(std::max<size_t>(fit, 1) * (size_t)th, (size_t)g.height + th);
    if (config.result_location == MemoryLocation::Device) {
        *st = Status::error(StatusCode::InvalidArgument,
            "pipeline: the grid's state (" + std::to_string(per_row * (size_t)g.height >> 20) + " MB) exceeds the device budget (" +
            std::to_string(budget >> 20) + " MB): it is processed out of core, which needs result_location = Host");
        return nullptr;
    }
    auto made = std::make_unique<Banded>();
    Banded& bd = *made;
    bd.cfg = config;
    bd.plan = detail::plan_groups(config);
    bd.spec_filters = filters.any();
    for (int r0 = 0; r0 < g.height; r0 += band_rows) bd.bands.push_back({r0, std::min(r0 + band_rows, g.height)});
    bd.parked.resize(bd.bands.size());
    bd.host_budget = config.host_cache_budget;
    if (bd.host_budget == 0) {
        long pages = sysconf(_SC_AVPHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
        bd.host_budget = pages > 0 && psz > 0 ? (size_t)pages * (size_t)psz / 2 : (size_t)8 << 30;
    }
    {
        std::error_code ec;
        const std::filesystem::path base = config.state_dir.empty() ? std::filesystem::temp_directory_path(ec)
                                                                    : std::filesystem::path(config.state_dir);
        bd.spill_dir = (base / ("pcr_spill_" + std::to_string((long long)getpid()) + "_" +
                                std::to_string((unsigned long long)(uintptr_t)owner))).string();
        std::filesystem::create_directories(bd.spill_dir, ec);
        if (ec) { *st = Status::error(StatusCode::IoError, "pipeline: cannot create " + bd.spill_dir); return nullptr; }
    }
    // the first band is created once here, so that an impossible configuration fails at create like an in-core one
    std::unique_ptr<Pipeline> probe = bd.visit(0, st);
    if (!probe) return nullptr;
    std::fprintf(stderr, "Info: grid state %zu MB exceeds the device budget %zu MB - out of core in %zu bands of %d rows\n",
                 per_row * (size_t)g.height >> 20, budget >> 20, bd.bands.size(), band_rows);
    probe.reset();
    if (config.resume && !config.state_dir.empty()) {
        // the tiles under state_dir are taken band by band (and, beyond the host budget, go back there: same files)
        if (!(*st = bd.load_state(config.state_dir)).ok()) return nullptr;
    }
    return made;
}

Pipeline::Banded::~Banded() {
    if (!spill_dir.empty()) {
        std::error_code ec;
        std::filesystem::remove_all(spill_dir, ec);
    }
}

// bytes of device memory one grid row costs: 4 B per cell and plane (a MostRecent group's packed words: 8 B per cell,
// its two slots), + the finalized bands a sub-pipeline keeps
size_t Pipeline::Banded::bytes_per_row(const PipelineConfig& c) {
    size_t planes = 0;
    for (const auto& gr : detail::plan_groups(c).groups)
        for (int p = 0; p < 4; ++p) planes += (gr.mask & kPlaneBits[p]) ? 1 : 0;
    // (PipelineConfig::histograms: a cube's bin planes and its percentile bands count like any other plane and band)
    for (const auto& h : c.histograms) planes += (size_t)std::max(h.bins, 0) + h.percentiles.size();
    // (PipelineConfig::extremes: k key planes and one band per entry)
    for (const auto& e : c.extremes) planes += (size_t)std::max(e.k, 0) + 1;
    // (PipelineConfig::cell_stats: 20 bytes of state per cell -- five 4-byte planes' worth -- and one band per product)
    for (const auto& s : c.cell_stats) planes += 5 + s.products.size();
    return (size_t)c.grid.width * 4 * (planes + c.reductions.size());
}

// a band nobody has touched yet: identity planes, no flags
void Pipeline::Banded::blank(size_t b, Parked& k) const {
    const size_t cells = (size_t)(bands[b].second - bands[b].first) * (size_t)cfg.grid.width;
    k.planes.assign(plan.groups.size() * 4, {});
    for (size_t g = 0; g < plan.groups.size(); ++g)
        for (int p = 0; p < 4; ++p)
            if (plan.groups[g].mask & kPlaneBits[p])
                k.planes[g * 4 + (size_t)p].assign(cells, detail::plane_identity(plan.groups[g].select, p));
    const GridConfig& g = cfg.grid;
    k.touched.assign((size_t)((g.width + g.tile_width - 1) / g.tile_width) * (size_t)((g.height + g.tile_height - 1) / g.tile_height), 0u);
}

Status Pipeline::Banded::spill(size_t b) {
    Parked& k = parked[b];
    Status s = detail::write_state_tiles(cfg.grid, plan.outputs, window_of(b, k), k.touched, spill_dir);
    if (!s.ok()) return s;
    host_used -= k.release();
    ++spills;
    return Status::success();
}

Status Pipeline::Banded::reload(size_t b) {
    Parked& k = parked[b];
    blank(b, k);
    size_t loaded = 0;
    Status s = detail::read_state_tiles(cfg.grid, plan.outputs, window_of(b, k), k.touched, spill_dir, &loaded);
    if (!s.ok()) return s;
    k.on_disk = false;
    host_used += k.bytes;
    ++reloads;
    return Status::success();
}

// park band b's state (already in k.planes / k.touched) and evict the least recently used bands beyond the host budget
Status Pipeline::Banded::account(size_t b) {
    Parked& k = parked[b];
    size_t bytes = k.touched.size() * 4;
    for (const auto& pl : k.planes) bytes += pl.size() * 4;
    host_used += bytes - (k.any && !k.on_disk ? k.bytes : 0);
    k.bytes = bytes;
    k.any = true;
    k.on_disk = false;
    k.stamp = ++clock;
    return evict();
}
Status Pipeline::Banded::evict() {
    while (host_used > host_budget) {
        size_t victim = parked.size();
        for (size_t i = 0; i < parked.size(); ++i)
            if (parked[i].any && !parked[i].on_disk && (victim == parked.size() || parked[i].stamp < parked[victim].stamp)) victim = i;
        if (victim == parked.size()) break;
        Status s = spill(victim);
        if (!s.ok()) return s;
    }
    return Status::success();
}

// was_on_disk: the band's state came from its files and those are still its current state
std::unique_ptr<Pipeline> Pipeline::Banded::visit(size_t b, Status* st, bool* was_on_disk) {
    PipelineConfig c = cfg;
    c.shard_row_begin = bands[b].first;
    c.shard_row_end = bands[b].second;
    c.result_location = MemoryLocation::Host;
    c.finalize_with_first_ingest = false;             // (a band's visit ends with its state parked, never with finalize)
    c.shard_halo_rows = -2;                           // whole tile rows: the band's state window is the band
    c.output_path.clear();
    c.fill_nodata_radius = 0;                         // (a band lacks its neighbours' rows: finalize() fills the assembled grid)
    c.ground = GroundFilterConfig();                  // (... and filters it)
    c.terrain.clear();                                // (... and derives the terrain bands)
    c.trees.clear();                                  // (... and the tree bands)
    c.state_dir.clear();
    c.resume = false;
    c.exec_mode = ExecutionMode::GPU;
    c.gpu_fallback_to_cpu = false;                    // (a band is a device pipeline or an error)
    if (was_on_disk) *was_on_disk = false;
    std::unique_ptr<Pipeline> sub = Pipeline::create(c);
    if (!sub) { *st = Status::error(StatusCode::OutOfMemory, "pipeline: out-of-core band could not be created: " + pipeline_create_error()); return nullptr; }
    Parked& k = parked[b];
    if (k.any) {
        if (k.on_disk) {
            if (!(*st = reload(b)).ok()) return nullptr;
            if (was_on_disk) *was_on_disk = true;
        }
        if (!(*st = sub->impl_->import_window(k.planes, k.touched)).ok()) return nullptr;
        k.stamp = ++clock;
    }
    *st = Status::success();
    return sub;
}

// Survivors of PipelineConfig::filter, as the bands' own ingests will count them (the same sweep on the same channels, class 0
// alone): what points_processed grows by (src/engine/pipeline.cpp:749), whether or not any band is visited.
Status Pipeline::Banded::count_kept(const PointCloud& dev, size_t* kept) {
    const size_t n = dev.count();
    Impl::DeviceScope scope(cfg.cuda_device_id);
    PipelineConfig alone;
    alone.filter = cfg.filter;
    detail::FilterPlan class0;
    Status s = detail::plan_filters(alone, &class0);
    detail::Buffer mb;
    if (s.ok()) s = mb.allocate(detail::filter_stage_bytes(class0, n), MemoryLocation::Device);
    if (!s.ok()) return s;
    std::vector<const uint8_t*> masks;
    return detail::sweep_filter_classes(class0, [&dev](const std::string& name, const float** out) {
        *out = static_cast<const float*>(dev.channel_data(name));
        return Status::success();
    }, n, mb.data(), nullptr, &masks, kept);
}

Status Pipeline::Banded::ingest(const PointCloud& cloud) {
    if (cloud.count() == 0) return Status::success();
    // the checks every band's ingest would make, made once and whether or not the cloud reaches a band
    Status ok = detail::validate_cloud(cfg, cloud, PCR_HIP_MAX_FILTER_SET, PCR_HIP_MAX_FILTER_PREDICATES);
    if (!ok.ok()) return ok;
    detail::Reprojection rp;
    if (!(ok = detail::plan_reprojection(cfg, cloud, &rp)).ok()) return ok;
    // one device copy of a host cloud for all bands (each band's kernels read every point and keep its own)
    std::unique_ptr<PointCloud> staged;
    const PointCloud* src = &cloud;
    if (cloud.location() != MemoryLocation::Device || rp.needed) {
        staged = cloud.to(MemoryLocation::Device);
        if (staged) src = staged.get();
        else if (rp.needed) return Status::error(StatusCode::OutOfMemory, "pipeline: cannot copy the cloud to the device for its reprojection");
    }
    // A cloud in another CRS than the grid's is transformed once, on that copy (the caller's cloud is only read); the
    // bands' sub-pipelines see it tagged with the grid's CRS and do not transform it again
    if (rp.needed) {
        Impl::DeviceScope dev(cfg.cuda_device_id);
        if (!(ok = detail::hip_status(pcr_hip_transform_xy(&rp.src, &rp.dst, staged->x(), staged->y(), staged->x(), staged->y(),
                                                           staged->count(), nullptr))).ok()) return ok;
        if (!(ok = detail::hip_status(pcr_hip_stream_synchronize(nullptr))).ok()) return ok;
        staged->set_crs(rp.dst_crs);
    }
    // points_processed counts the filter's survivors (round 5's fuzz: it counted the cloud); none: nothing to do, and the
    // ingest is not a collection either (src/engine/pipeline.cpp:349-353)
    size_t kept = cloud.count();
    bool kept_known = cfg.filter.empty();
    if (!kept_known && src->location() == MemoryLocation::Device) {
        if (!(ok = count_kept(*src, &kept)).ok()) return ok;
        kept_known = true;
        if (kept == 0) return Status::success();
    }
    // Which bands does this cloud reach at all?  One routing pass over x, y (pcr_hip_route_count with the bands as the parts:
    // 16 B per point, ~0.2 ms per 100 M points) against ~50 ms per band VISITED (a sub-pipeline, the band's state over
    // PCIe both ways: profiles/r05_out_of_core_cost.md) -- a survey tile that covers a corner of the grid then costs its
    // own bands only.  (The filter is not applied: a superset of the kept points, so no band is skipped wrongly.)
    std::vector<uint64_t> reach(bands.size(), 1);
    size_t valid_total = 0;
    if (bands.size() <= PCR_HIP_MAX_ROUTE_PARTS && src->location() == MemoryLocation::Device) {
        Impl::DeviceScope dev(cfg.cuda_device_id);
        const pcr_hip_grid hg = detail::to_hip_grid(cfg.grid);
        std::vector<int32_t> splits;
        for (const auto& bd : bands) splits.push_back(bd.first);
        splits.push_back(bands.back().second);
        detail::Buffer dest, counts;
        std::vector<uint64_t> host(bands.size(), 0);
        if (dest.allocate(src->count(), MemoryLocation::Device).ok() && counts.allocate(bands.size() * 8, MemoryLocation::Device).ok() &&
            pcr_hip_route_count(&hg, splits.data(), (int)bands.size(), src->x(), src->y(), nullptr, src->count(),
                                static_cast<uint8_t*>(dest.data()), static_cast<unsigned long long*>(counts.data()), nullptr) == PCR_HIP_OK &&
            pcr_hip_memcpy_d2h(host.data(), counts.data(), host.size() * 8, nullptr) == PCR_HIP_OK &&
            pcr_hip_stream_synchronize(nullptr) == PCR_HIP_OK)
            reach = host;
    }
    for (size_t b = 0; b < bands.size(); ++b) {
        if (reach[b] == 0) continue;                                    // none of this cloud's points has its centre row here
        Status s = Status::success();
        bool from_disk = false;
        std::unique_ptr<Pipeline> sub = visit(b, &s, &from_disk);
        if (!sub) return s;
        if (!(s = sub->ingest(*src)).ok()) return s;                    // returns mid-loop, earlier bands keep the cloud
        if (!kept_known) { kept = (size_t)sub->stats().points_processed; kept_known = true; }   // (a fresh sub-pipeline: this ingest's survivors)
        const ScatterInfo here = sub->last_scatter();
        valid_total += here.points_valid;
        last = here;
        // With spec filters the last scatter's count is its own class's: a group before it, or the touched flags, may have
        // taken points where it took none -- every band the cloud reaches counts as changed then
        const bool changed = here.points_valid != 0 || spec_filters;
        if (!parked[b].any && !changed) continue;                        // nothing of this cloud (or any before) fell here
        Parked& k = parked[b];
        if (!changed && k.any) {                                         // unchanged: the parked copy (and its files) stay current
            if (from_disk) drop_host_copy(b);
            else if (!(s = evict()).ok()) return s;
            continue;
        }
        if (!(s = sub->impl_->export_window(k.planes, k.touched)).ok()) return s;
        if (!(s = account(b)).ok()) return s;
    }
    last.points_in = cloud.count();                                     // (of the whole ingest: every band saw every point)
    last.points_valid = valid_total;
    ++collections;
    points += kept;
    if (callback) {
        ProgressInfo info = stats();
        if (!callback(info)) return Status::error(StatusCode::InvalidArgument, "pipeline: cancelled by user");
    }
    return Status::success();
}

Status Pipeline::Banded::finalize() {
    const GridConfig& g = cfg.grid;
    std::vector<BandDesc> descs;
    for (const auto& r : cfg.reductions) {
        BandDesc d;
        d.name = detail::default_band_name(r);
        d.dtype = DataType::Float32;
        d.is_state = false;
        descs.push_back(d);
    }
    if (descs.empty()) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate result grid");
    detail::GroundPlan ground;
    Status gs = detail::plan_ground(cfg, &ground);
    if (!gs.ok()) return gs;
    detail::TerrainPlan terrain;
    if (!(gs = detail::plan_terrain(cfg, ground, &terrain)).ok()) return gs;
    detail::TreesPlan trees;
    if (!(gs = detail::plan_trees(cfg, ground, terrain, &trees)).ok()) return gs;
    const size_t n_out = descs.size();                // (the ground filter's and the terrain bands follow: no band visit makes them)
    detail::append_ground_bands(ground, descs);
    detail::append_terrain_bands(terrain, descs);
    detail::append_tree_bands(trees, descs);
    if (!result) result = Grid::create(g.width, g.height, descs, MemoryLocation::Host);
    if (!result) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate result grid");
    (void)result->set_geometry(detail::result_geometry(cfg));
    tiles_active = 0;
    for (size_t b = 0; b < bands.size(); ++b) {
        Status s = Status::success();
        if (!parked[b].any) {
            // no point ever had its centre row here: every tile of the band is untouched, every band NaN (Q3) -- no visit
            const size_t first = (size_t)bands[b].first * g.width, cells = (size_t)(bands[b].second - bands[b].first) * g.width;
            for (size_t o = 0; o < n_out; ++o)
                std::fill_n(result->band_f32((int)o) + first, cells, std::numeric_limits<float>::quiet_NaN());
            continue;
        }
        bool from_disk = false;
        std::unique_ptr<Pipeline> sub = visit(b, &s, &from_disk);
        if (!sub) return s;
        if (!(s = sub->finalize()).ok()) return s;
        const Grid* part = sub->result();
        const int rows = bands[b].second - bands[b].first;
        if (!part || part->rows() != rows) return Status::error(StatusCode::CudaError, "pipeline: out-of-core band returned no result");
        for (size_t o = 0; o < n_out; ++o)
            std::copy_n(part->band_f32((int)o), (size_t)rows * g.width, result->band_f32((int)o) + (size_t)bands[b].first * g.width);
        for (uint32_t t : parked[b].touched) tiles_active += t ? 1 : 0;
        // finalize changes no state: a band that was read back from its files goes back to being "on disk" at once, and
        // the host budget holds during finalize as it does during ingest (it used to end with every band in RAM)
        if (from_disk) drop_host_copy(b);
        else if (!(s = evict()).ok()) return s;
    }
    {                                                 // the result is assembled here, on the host: so are its ground filter and its fill
        std::vector<ReductionType> types;
        for (const auto& r : cfg.reductions) types.push_back(r.type);
        Status fs = detail::finish_result_host(*result, types, cfg.fill_nodata_radius, ground, terrain, trees, &tree_tables, &tree_status);
        if (!fs.ok()) return fs;
    }
    finalized = true;
    if (!cfg.output_path.empty()) return write_geotiff(cfg.output_path, *result, cfg.grid, pipeline_output_options(cfg.write_cog));
    return Status::success();
}

// ---- `.pcrt` checkpoints of the whole pipeline: every band's tiles under `dir` (the in-core pipeline's layout)
Status Pipeline::Banded::save_state(const std::string& dir_in) {
    const std::string dir = dir_in.empty() ? cfg.state_dir : dir_in;
    if (dir.empty()) return Status::error(StatusCode::InvalidArgument, "pipeline: no state directory given");
    for (size_t b = 0; b < bands.size(); ++b) {
        Parked& k = parked[b];
        if (!k.any) continue;
        bool from_disk = false;
        Status s = Status::success();
        if (k.on_disk) {
            if (!(s = reload(b)).ok()) return s;
            from_disk = true;
        }
        if (!(s = detail::write_state_tiles(cfg.grid, plan.outputs, window_of(b, k), k.touched, dir)).ok()) return s;
        if (from_disk) drop_host_copy(b);
    }
    return Status::success();
}

Status Pipeline::Banded::load_state(const std::string& dir_in) {
    const std::string dir = dir_in.empty() ? cfg.state_dir : dir_in;
    if (dir.empty()) return Status::error(StatusCode::InvalidArgument, "pipeline: no state directory given");
    for (size_t b = 0; b < bands.size(); ++b) {
        Parked& k = parked[b];
        Status s = Status::success();
        Parked fresh;
        Parked* into = &k;
        if (k.any) {
            if (k.on_disk && !(s = reload(b)).ok()) return s;           // files overlay the band's current state, as in core
        } else {
            blank(b, fresh);
            into = &fresh;
        }
        size_t loaded = 0;
        if (!(s = detail::read_state_tiles(cfg.grid, plan.outputs, window_of(b, *into), into->touched, dir, &loaded)).ok()) return s;
        if (!loaded) continue;                                          // a reloaded band stays in host memory here
        if (into == &fresh) { k.planes = std::move(fresh.planes); k.touched = std::move(fresh.touched); }
        if (!(s = account(b)).ok()) return s;
    }
    return Status::success();
}

ProgressInfo Pipeline::Banded::stats() const {
    ProgressInfo info;
    info.collections_processed = collections;
    info.points_processed = points;
    info.tiles_active = tiles_active;
    info.elapsed_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
    return info;
}

}  // namespace pcr
