// device_pipeline.cpp -- Pipeline::Impl (device_pipeline.h): the in-core pipeline on the HIP engine.
//   * no router / sort / per-tile batches / tile manager: reductions that read the same value channel through the same glyph
//     share ONE pass over the points and ONE set of device planes (sum, weight, max, min);
//   * finalize runs on the device; only finalized bands cross PCIe (or stay in HBM).
#include "device_pipeline.h"

#include "fill_nodata.h"
#include "ground_filter.h"
#include "overviews.h"
#include "polygonize.h"
#include "pcr/core/point_cloud.h"
#include "pcr/io/grid_io.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <mutex>
#include <set>

namespace pcr {

using detail::kPlaneBits;

Pipeline::Impl::~Impl() {
    if (engine) pcr_hip_engine_destroy(engine);
    surfaces.clear();
    polygon_sets.clear();
    cubes.clear();
    ext_keys.clear();
    stat_planes.clear();
    groups.clear();
    bands.clear();
    band_buffers.clear();
    d_ground_work.release();
    d_tree_work.clear();
    zone_grids.clear();
    pz_state.tables.clear();
    staging.clear();
    result.reset();
    if (own_stream && stream) pcr_hip_stream_destroy(stream);
}

Status Pipeline::Impl::init() {
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
        if (!ok.ok()) return ok;
    }

    // The reference's GPU-initialisation matrix (src/engine/pipeline.cpp:108-162), with its exact messages and status
    // codes.  Where the reference goes on in CPU mode it prints a Warning / Info line on stderr first; so does this build,
    // and then Pipeline::create continues on the host engine (host_pipeline.h) -- never silently: the line is printed, and
    // Pipeline::engine() says which engine a pipeline runs on.  PCR_REQUIRE_GPU_ENGINE=1 in the environment turns every
    // such fallback into an error (GPU test suites and benchmarks set it: a CPU result must not pass for a GPU one).
    auto no_cpu_engine = [this](const char* how) {
        continue_on_host = true;
        return Status::error(StatusCode::NotImplemented,
            std::string("pipeline: ") + how + ", and PCR_REQUIRE_GPU_ENGINE forbids it");
    };
    int ndev = 0;
    pcr_hip_device_count(&ndev);
    if (ndev <= 0) {
        const std::string msg = "No CUDA-capable GPU detected";
        if (cfg.exec_mode != ExecutionMode::GPU) {                                                  // Auto, Hybrid
            std::fprintf(stderr, "Info: %s - using CPU mode\n", msg.c_str());                       // pipeline.cpp:130
            return no_cpu_engine("no GPU was found and the reference would use its CPU mode");
        }
        if (cfg.gpu_require_strict)
            return Status::error(StatusCode::CudaError, msg + " - GPU mode requested but no GPU available");   // :118-119
        if (cfg.gpu_fallback_to_cpu) {
            std::fprintf(stderr, "Warning: %s - falling back to CPU mode\n", msg.c_str());          // :122
            return no_cpu_engine("the reference would fall back to its CPU mode here");
        }
        return Status::error(StatusCode::CudaError, msg + " - GPU required but not available");         // :125-126
    }
    Status s = Status::success();
    if (cfg.cuda_device_id >= 0) {
        const int rc = cfg.cuda_device_id < ndev ? pcr_hip_set_device(cfg.cuda_device_id) : PCR_HIP_INVALID_ARGUMENT;
        if (rc != PCR_HIP_OK) {
            const std::string err_msg = "Failed to set CUDA device " + std::to_string(cfg.cuda_device_id) + ": " +
                                        (cfg.cuda_device_id < ndev ? std::string(pcr_hip_last_error()) : std::string("invalid device ordinal"));   // :136-137
            if (cfg.gpu_require_strict) return Status::error(StatusCode::CudaError, err_msg);          // :141
            if (cfg.gpu_fallback_to_cpu) {
                std::fprintf(stderr, "Warning: %s - falling back to CPU mode\n", err_msg.c_str());   // :143
                return no_cpu_engine("the reference would fall back to its CPU mode here");
            }
            return Status::error(StatusCode::CudaError, err_msg);                                      // :146
        }
    } else {
        return Status::error(StatusCode::InvalidArgument, "pipeline: invalid device id");
    }
    {
        // pipeline.cpp:149-160, once per device and process (the reference prints it at every create; a bench that
        // creates a pipeline per step would bury its own output)
        static std::mutex mu;
        static std::set<int> announced;
        std::lock_guard<std::mutex> lock(mu);
        if (announced.insert(cfg.cuda_device_id).second) {
            const std::string name = cuda_device_name(cfg.cuda_device_id);
            size_t free_mem = 0, total_mem = 0;
            if (cuda_get_memory_info(&free_mem, &total_mem, cfg.cuda_device_id))
                std::fprintf(stderr, "Info: Using GPU %d: %s (%.1f GB free / %.1f GB total)\n", cfg.cuda_device_id, name.c_str(),
                             free_mem / (1024.0 * 1024.0 * 1024.0), total_mem / (1024.0 * 1024.0 * 1024.0));
            else
                std::fprintf(stderr, "Info: Using GPU %d: %s\n", cfg.cuda_device_id, name.c_str());
        }
    }
    if (cfg.use_cuda_streams) {
        s = detail::hip_status(pcr_hip_stream_create(&stream));
        if (!s.ok()) return s;
        own_stream = true;
    }

    // accumulation groups + outputs (the percentile bands behind the reductions' and ahead of the DTM, hag and terrain bands)
    {
        detail::GroupPlan plan = detail::plan_groups(cfg);
        groups.resize(plan.groups.size());
        for (size_t gi = 0; gi < groups.size(); ++gi) static_cast<detail::GroupSpec&>(groups[gi]) = plan.groups[gi];
        outputs = std::move(plan.outputs);
    }
    hist = detail::plan_histograms(cfg, filters);
    ext = detail::plan_extremes(cfg, filters);
    cstats = detail::plan_cell_stats(cfg, filters);
    if (!(s = detail::plan_ground(cfg, &ground)).ok()) return s;
    if (!(s = detail::plan_terrain(cfg, ground, &terrain)).ok()) return s;
    if (!(s = detail::plan_trees(cfg, ground, terrain, &tree_plan)).ok()) return s;
    if (!(s = detail::plan_zonal(cfg, ground, terrain, tree_plan, &zonal_plan)).ok()) return s;
    if (!(s = detail::plan_surfaces(cfg)).ok()) return s;
    surfaces.resize(cfg.surface_channels.size());
    if (!(s = detail::plan_polygon_channels(cfg)).ok()) return s;
    polygon_sets.resize(cfg.polygon_channels.size());

    // row window of this device
    int r0 = 0, r1 = g.height;
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0) {
        r0 = cfg.shard_row_begin < 0 ? 0 : cfg.shard_row_begin;
        r1 = cfg.shard_row_end < 0 ? g.height : cfg.shard_row_end;
        if (r0 > r1 || r1 > g.height)
            return Status::error(StatusCode::InvalidArgument, "pipeline: shard row range outside the grid");
        for (const auto& gr : groups) halo = std::max(halo, reach_rows(gr.glyph));
        halo = std::max(halo, cfg.shard_halo_rows);
        halo = std::min(halo, g.height);
        // -2 (the out-of-core bands): the block is made of whole reference-tile rows, footprints are clipped to the tile
        // of their centre cell (Q4), nothing can land outside the block -- no apron rows at all
        if (cfg.shard_halo_rows == -2 && r0 % g.tile_height == 0 && (r1 % g.tile_height == 0 || r1 == g.height)) halo = 0;
    }
    hg = detail::to_hip_grid(g);
    hg.own_row0 = r0; hg.own_row1 = r1;
    hg.state_row0 = std::max(0, r0 - halo);
    hg.state_rows = std::min(g.height, r1 + halo) - hg.state_row0;

    {
        // arena pre-sized at create, like the reference's MemoryPool; a pool that cannot be created follows the
        // reference's matrix too (src/engine/pipeline.cpp:181-192)
        const int rc = pcr_hip_engine_create(&engine, &hg, cfg.gpu_pool_size_bytes, stream);
        if (rc == PCR_HIP_OUT_OF_MEMORY) {
            const std::string err_msg = "Failed to create GPU memory pool";
            if (cfg.gpu_require_strict || !cfg.gpu_fallback_to_cpu) return Status::error(StatusCode::OutOfMemory, err_msg);
            std::fprintf(stderr, "Warning: %s - falling back to CPU mode\n", err_msg.c_str());
            return no_cpu_engine("the reference would fall back to its CPU mode here");
        }
        s = detail::hip_status(rc);
        if (!s.ok()) return s;
    }
    s = detail::hip_status(pcr_hip_engine_set_path(engine, cfg.scatter_path));
    if (!s.ok()) return s;

    const int64_t cells = (int64_t)hg.state_rows * hg.width;
    for (auto& gr : groups) {
        if (gr.select) {
            s = gr.packed.allocate((size_t)std::max<int64_t>(cells, 1) * sizeof(uint64_t), MemoryLocation::Device);
            if (!s.ok()) return s;
            continue;
        }
        for (int p = 0; p < 4; ++p) {
            if (!(gr.mask & kPlaneBits[p])) continue;
            s = gr.planes[p].allocate((size_t)std::max<int64_t>(cells, 1) * sizeof(float), MemoryLocation::Device);
            if (!s.ok()) return s;
        }
        gr.view.d_sum = static_cast<float*>(gr.planes[0].data());
        gr.view.d_wgt = static_cast<float*>(gr.planes[1].data());
        gr.view.d_max = static_cast<float*>(gr.planes[2].data());
        gr.view.d_min = static_cast<float*>(gr.planes[3].data());
    }
    cubes.resize(hist.entries.size());
    for (size_t h = 0; h < cubes.size(); ++h) {
        const size_t bytes = hist.entries[h].cube_cells((size_t)std::max<int64_t>(cells, 1)) * sizeof(uint32_t);
        if (!(s = cubes[h].allocate(bytes, MemoryLocation::Device)).ok()) return s;
        if (!(s = detail::hip_status(pcr_hip_memset(cubes[h].data(), 0, bytes, stream))).ok()) return s;
    }
    ext_keys.resize(ext.entries.size());
    for (size_t x = 0; x < ext_keys.size(); ++x) {                // every slot EMPTY (0xFFFFFFFF)
        const size_t bytes = ext.entries[x].state_cells((size_t)std::max<int64_t>(cells, 1)) * sizeof(uint32_t);
        if (!(s = ext_keys[x].allocate(bytes, MemoryLocation::Device)).ok()) return s;
        if (!(s = detail::hip_status(pcr_hip_memset(ext_keys[x].data(), 0xFF, bytes, stream))).ok()) return s;
    }
    stat_planes.resize(cstats.entries.size());
    for (auto& p : stat_planes) {                                 // all zero
        const size_t c = (size_t)std::max<int64_t>(cells, 1);
        detail::Buffer* bufs[3] = {&p.n, &p.s1, &p.s2};
        const size_t bytes[3] = {c * sizeof(uint32_t), c * sizeof(int64_t), c * sizeof(uint64_t)};
        for (int k = 0; k < 3; ++k) {
            if (!(s = bufs[k]->allocate(bytes[k], MemoryLocation::Device)).ok()) return s;
            if (!(s = detail::hip_status(pcr_hip_memset(bufs[k]->data(), 0, bytes[k], stream))).ok()) return s;
        }
    }
    if (!(s = pz_state.allocate(pz_plan, MemoryLocation::Device, stream)).ok()) return s;     // PipelineConfig::point_zonal: all zero
    if (!outputs.empty() && !(s = allocate_result()).ok()) return s;
    if (!(s = d_bands_done.allocate(std::max<size_t>(groups.size(), 1) * sizeof(uint32_t), MemoryLocation::HostPinned)).ok()) return s;
    std::memset(d_bands_done.data(), 0, d_bands_done.bytes());
    return detail::hip_status(pcr_hip_stream_synchronize(stream));
}

// The slot (0 Sum, 1 Count, 2 Max, 3 Min) of the plane a reduction finalizes unchanged; -1: none.
int Pipeline::Impl::own_plane(ReductionType t) {
    return t == ReductionType::Sum ? 0 : t == ReductionType::Count ? 1 : t == ReductionType::Max ? 2 : t == ReductionType::Min ? 3 : -1;
}
// Band b of the table leaves the pipeline, behind whatever stored its raw self on the pipeline's stream: a filled band is
// filled from `raw` into `out`, and a host-resident result gets its copy of `out`.
Status Pipeline::Impl::band_leaves(size_t b, bool* enqueued) {
    const int rows = own_rows(), W = hg.width;
    const LeavingBand& lb = bands[b];
    Status s = Status::success();
    if (lb.out != lb.raw) {
        *enqueued = true;
        s = detail::hip_status(pcr_hip_fill_nodata(lb.raw, lb.out, W, rows, W, W, cfg.fill_nodata_radius, stream));
        if (!s.ok()) return s;
    }
    if (cfg.result_location != MemoryLocation::Device) {
        *enqueued = true;
        s = detail::hip_status(pcr_hip_memcpy_d2h(result->band_f32((int)b), lb.out, (size_t)rows * W * sizeof(float), stream));
    }
    return s;
}
// Behind the finalize kernels of every group, on the pipeline's stream, and ahead of the ground filter, which may read a
// percentile band: one walk per histogram writes all of its raw bands, which then leave like a Max band (filled when asked).
Status Pipeline::Impl::finalize_histograms(bool* enqueued) {
    size_t r = cfg.reductions.size();
    for (size_t h = 0; h < hist.entries.size(); ++h) {
        const detail::HistogramEntry& e = hist.entries[h];
        if (e.q.empty()) continue;
        std::vector<float*> dsts;
        for (size_t j = 0; j < e.q.size(); ++j) dsts.push_back(bands[r + j].raw);
        *enqueued = true;
        Status s = detail::hip_status(pcr_hip_histogram_percentiles(&hg, static_cast<const uint32_t*>(cubes[h].data()), e.bins, e.lo, e.w,
                                                                    (int)e.q.size(), e.q.data(), dsts.data(), stream));
        for (size_t j = 0; j < e.q.size() && s.ok(); ++j) s = band_leaves(r + j, enqueued);
        if (!s.ok()) return s;
        r += e.q.size();
    }
    return Status::success();
}
// The cube of histogram i as a host copy, behind everything on the pipeline's stream.
Status Pipeline::Impl::histogram_counts(int i, std::vector<uint32_t>* out) {
    if (i < 0 || (size_t)i >= cubes.size() || !out)
        return Status::error(StatusCode::InvalidArgument, "pipeline: histogram_counts: no histogram " + std::to_string(i));
    DeviceScope dev(cfg.cuda_device_id);
    out->assign(hist.entries[(size_t)i].cube_cells((size_t)hg.state_rows * hg.width), 0u);
    if (out->empty()) return Status::success();
    Status s = detail::hip_status(pcr_hip_memcpy_d2h(out->data(), cubes[(size_t)i].data(), out->size() * sizeof(uint32_t), stream));
    return s.ok() ? detail::hip_status(pcr_hip_stream_synchronize(stream)) : s;
}
// Behind the percentile bands and ahead of the ground filter, which may read an extremes band ("z_low"): one walk per entry
// writes its raw band, which then leaves like a Min (Lowest) or Max (Highest) band (filled when asked).
Status Pipeline::Impl::finalize_extremes(bool* enqueued) {
    size_t r = cfg.reductions.size() + (size_t)hist.extra_bands();
    for (size_t x = 0; x < ext.entries.size(); ++x, ++r) {
        const detail::ExtremesEntry& e = ext.entries[x];
        *enqueued = true;
        Status s = detail::hip_status(pcr_hip_extremes_band(&hg, static_cast<const uint32_t*>(ext_keys[x].data()), e.k, e.side, e.max_gap,
                                                            bands[r].raw, nullptr, stream));
        if (s.ok()) s = band_leaves(r, enqueued);
        if (!s.ok()) return s;
    }
    return Status::success();
}
// The values entry i keeps as a host copy, [k][rows * width], behind everything on the pipeline's stream: decoded on the device
// by the band kernel into memory of the call's own (the band it also writes is dropped).
Status Pipeline::Impl::extremes_values(int i, std::vector<float>* out) {
    if (i < 0 || (size_t)i >= ext_keys.size() || !out)
        return Status::error(StatusCode::InvalidArgument, "pipeline: extremes_values: no extremes entry " + std::to_string(i));
    DeviceScope dev(cfg.cuda_device_id);
    const detail::ExtremesEntry& e = ext.entries[(size_t)i];
    const size_t cells = (size_t)std::max(own_rows(), 0) * (size_t)hg.width;
    out->assign(e.state_cells(cells), 0.0f);
    if (out->empty()) return Status::success();
    detail::Buffer d_tmp;                                         // [band][k value planes]
    Status s = d_tmp.allocate((e.state_cells(cells) + cells) * sizeof(float), MemoryLocation::Device);
    if (!s.ok()) return s;
    float* d_band = static_cast<float*>(d_tmp.data());
    s = detail::hip_status(pcr_hip_extremes_band(&hg, static_cast<const uint32_t*>(ext_keys[(size_t)i].data()), e.k, e.side, e.max_gap,
                                                 d_band, d_band + cells, stream));
    if (s.ok()) s = detail::hip_status(pcr_hip_memcpy_d2h(out->data(), d_band + cells, out->size() * sizeof(float), stream));
    const Status w = detail::hip_status(pcr_hip_stream_synchronize(stream));      // (d_tmp is released behind the kernel)
    return s.ok() ? w : s;
}
// Behind the extremes' bands and ahead of the ground filter, which may read a cell-stats band ("z_mean"): one launch per entry
// writes all of its raw bands; a Mean band then leaves like an Average band (filled when asked), the spread bands as they are.
Status Pipeline::Impl::finalize_cell_stats(bool* enqueued) {
    size_t r = cfg.reductions.size() + (size_t)hist.extra_bands() + (size_t)ext.extra_bands();
    for (size_t x = 0; x < cstats.entries.size(); ++x) {
        const detail::CellStatsEntry& e = cstats.entries[x];
        std::vector<float*> dsts;
        for (size_t j = 0; j < e.products.size(); ++j) dsts.push_back(bands[r + j].raw);
        *enqueued = true;
        Status s = detail::hip_status(pcr_hip_cell_stats_bands(&hg, static_cast<const uint32_t*>(stat_planes[x].n.data()),
                                                               static_cast<const long long*>(stat_planes[x].s1.data()),
                                                               static_cast<const unsigned long long*>(stat_planes[x].s2.data()), e.origin,
                                                               e.resolution, e.ddof, (int)e.products.size(), e.products.data(), dsts.data(),
                                                               stream));
        for (size_t j = 0; j < e.products.size() && s.ok(); ++j) s = band_leaves(r + j, enqueued);
        if (!s.ok()) return s;
        r += e.products.size();
    }
    return Status::success();
}
// The three planes of entry i as host copies, behind everything on the pipeline's stream.
Status Pipeline::Impl::cell_stats_state(int i, std::vector<uint32_t>* n, std::vector<int64_t>* s1, std::vector<uint64_t>* s2) {
    if (i < 0 || (size_t)i >= stat_planes.size() || !n || !s1 || !s2)
        return Status::error(StatusCode::InvalidArgument, "pipeline: cell_stats_state: no cell_stats entry " + std::to_string(i));
    DeviceScope dev(cfg.cuda_device_id);
    const size_t cells = (size_t)hg.state_rows * hg.width;
    n->assign(cells, 0u);
    s1->assign(cells, 0);
    s2->assign(cells, 0u);
    if (cells == 0) return Status::success();
    const StatPlanes& p = stat_planes[(size_t)i];
    Status s = detail::hip_status(pcr_hip_memcpy_d2h(n->data(), p.n.data(), cells * sizeof(uint32_t), stream));
    if (s.ok()) s = detail::hip_status(pcr_hip_memcpy_d2h(s1->data(), p.s1.data(), cells * sizeof(int64_t), stream));
    if (s.ok()) s = detail::hip_status(pcr_hip_memcpy_d2h(s2->data(), p.s2.data(), cells * sizeof(uint64_t), stream));
    const Status w = detail::hip_status(pcr_hip_stream_synchronize(stream));
    return s.ok() ? w : s;
}
// Behind the finalize kernels and the fills of every group, on the pipeline's stream: the filter on the RAW source band, the
// DTM leaves (filled like a Min band), hag from the top band and the DTM as they leave the pipeline, hag leaves.
Status Pipeline::Impl::finalize_ground(bool* enqueued) {
    if (!ground.on) return Status::success();
    const int rows = own_rows(), W = hg.width;
    const size_t dtm = outputs.size(), hag = dtm + 1;
    size_t bytes = 0;
    Status s = detail::hip_status(pcr_hip_ground_filter_work_bytes(W, rows, &bytes));
    if (!s.ok()) return s;
    if (d_ground_work.bytes() < bytes && !(s = d_ground_work.allocate(bytes, MemoryLocation::Device)).ok()) return s;
    *enqueued = true;
    s = detail::hip_status(pcr_hip_ground_filter(bands[(size_t)ground.source].raw, bands[dtm].raw, W, rows, W, W,
                                                 (int)ground.radii.size(), ground.radii.data(), ground.thresholds.data(),
                                                 d_ground_work.data(), d_ground_work.bytes(), stream));
    if (!s.ok()) return s;
    if (!(s = band_leaves(dtm, enqueued)).ok() || ground.top < 0) return s;
    s = detail::hip_status(pcr_hip_band_difference(bands[(size_t)ground.top].out, bands[dtm].out, bands[hag].raw, W, rows, W, W, W,
                                                   stream));
    return s.ok() ? band_leaves(hag, enqueued) : s;
}
// Behind everything that makes a source band, on the pipeline's stream: one launch per group of entries, reading the source
// band as it leaves the pipeline (`out`: filled) and storing the new bands, which then leave as they are.
Status Pipeline::Impl::finalize_terrain(bool* enqueued) {
    const int rows = own_rows(), W = hg.width;
    const size_t first = outputs.size() + (size_t)ground.extra_bands();
    for (const auto& l : terrain.launches) {
        const auto& f = terrain.bands[(size_t)l.front()];
        const TerrainSpec& spec = terrain.spec_of(l);
        const TerrainLight light = terrain_light((double)spec.azimuth, (double)spec.altitude);
        std::vector<int> products;
        std::vector<float*> dsts;
        std::vector<int64_t> strides;
        for (int m : l) {
            products.push_back(terrain.bands[(size_t)m].product);
            dsts.push_back(bands[first + (size_t)m].raw);
            strides.push_back(W);
        }
        *enqueued = true;
        Status s = detail::hip_status(pcr_hip_terrain(bands[(size_t)f.source].out, W, rows, W, (int)l.size(), products.data(),
                                                      dsts.data(), strides.data(), terrain.cell_size_x, terrain.cell_size_y,
                                                      (double)f.spec.z_factor, f.spec.compute_edges ? 1 : 0, light.sin_alt, light.ls,
                                                      light.lc, stream));
        for (int m : l)
            if (s.ok()) s = band_leaves(first + (size_t)m, enqueued);
        if (!s.ok()) return s;
    }
    return Status::success();
}
// Behind the terrain bands, on the pipeline's stream: per entry everything pcr_hip_trees enqueues, reading the source band as it
// leaves the pipeline (`out`: filled) and storing the two new bands, which then leave as they are.  No plane-state event.
Status Pipeline::Impl::finalize_trees(bool* enqueued) {
    const int rows = own_rows(), W = hg.width;
    const size_t first = outputs.size() + (size_t)ground.extra_bands() + (size_t)terrain.extra_bands();
    if (d_tree_work.size() < tree_plan.entries.size()) d_tree_work.resize(tree_plan.entries.size());
    for (size_t i = 0; i < tree_plan.entries.size(); ++i) {
        const auto& e = tree_plan.entries[i];
        size_t bytes = 0;
        Status s = detail::hip_status(pcr_hip_trees_work_bytes(W, rows, &bytes));
        if (!s.ok()) return s;
        if (d_tree_work[i].bytes() < bytes && !(s = d_tree_work[i].allocate(bytes, MemoryLocation::Device)).ok()) return s;
        const pcr_hip_tree_params p = detail::tree_params(e.spec, tree_plan.cell_size_x, tree_plan.cell_size_y);
        const size_t id = first + 2 * i, height = id + 1;
        *enqueued = true;
        s = detail::hip_status(pcr_hip_trees(bands[(size_t)e.source].out, W, rows, W, &p, bands[id].raw, W, bands[height].raw, W,
                                             d_tree_work[i].data(), d_tree_work[i].bytes(), stream));
        if (s.ok()) s = band_leaves(id, enqueued);
        if (s.ok()) s = band_leaves(height, enqueued);
        if (!s.ok()) return s;
    }
    return Status::success();
}
// The table of entry i as the last finalize left it in the entry's work area, behind everything on the pipeline's stream.
Status Pipeline::Impl::trees(int i, TreeTable* out) {
    if (!out || i < 0 || !finalized || !result || (size_t)i >= tree_plan.entries.size() || (size_t)i >= d_tree_work.size())
        return Status::error(StatusCode::InvalidArgument, "pipeline: trees: no trees entry " + std::to_string(i) + " (of a finalize)");
    DeviceScope dev(cfg.cuda_device_id);
    const auto& e = tree_plan.entries[(size_t)i];
    Status s = detail::tree_table_device(bands[(size_t)e.source].out, hg.width, own_rows(), hg.width, d_tree_work[(size_t)i].data(),
                                         d_tree_work[(size_t)i].bytes(), stream, out);
    if (s.ok()) detail::tree_centres(*out, result->geometry(), tree_plan.cell_size_x, tree_plan.cell_size_y);
    return s;
}
// PipelineConfig::zonal: the label band of an external entry into HBM the pipeline owns, behind everything on the stream.
Status Pipeline::Impl::set_zones(const std::string& name, const Grid& grid, int band) {
    DeviceScope dev(cfg.cuda_device_id);
    Status s = detail::hip_status(pcr_hip_stream_synchronize(stream));
    return s.ok() ? detail::store_zones(cfg, name, grid, band, MemoryLocation::Device, stream, &zone_grids) : s;
}
// ... or burnt there from polygons, on the pipeline's stream.
Status Pipeline::Impl::set_zones(const std::string& name, const PolygonSet& polygons, const RasterizeOptions& options) {
    DeviceScope dev(cfg.cuda_device_id);
    return detail::store_zones(cfg, name, polygons, options, MemoryLocation::Device, stream, &zone_grids);
}
// The table of entry i, behind the last finalize on the pipeline's stream: the label band as it left the pipeline (`out`), the
// cell-stats planes and the cubes where they are.  Nothing of it runs in finalize: no plane-state event.
Status Pipeline::Impl::zonal(int i, ZonalTable* out, bool with_counts) {
    if (!out || i < 0 || !finalized || !zonal_fresh || !result || (size_t)i >= zonal_plan.entries.size())
        return Status::error(StatusCode::InvalidArgument,
                             "pipeline: zonal: no zonal entry " + std::to_string(i) + " (of a finalize with no ingest since)");
    const auto& e = zonal_plan.entries[(size_t)i];
    detail::ZonalInputs in;
    in.device = true;
    in.stream = stream;
    in.width = hg.width;
    in.rows = own_rows();
    if (e.band >= 0) {
        in.zones = bands[(size_t)e.band].out;
    } else {
        const auto it = zone_grids.find(e.zones);
        if (it == zone_grids.end())
            return Status::error(StatusCode::InvalidArgument, "pipeline: zonal: the label grid '" + e.zones + "' was not set (set_zones)");
        in.zones = static_cast<const float*>(it->second.band.data());
    }
    for (const auto& p : stat_planes)
        in.stats.push_back({static_cast<const uint32_t*>(p.n.data()), static_cast<const long long*>(p.s1.data()),
                            static_cast<const unsigned long long*>(p.s2.data())});
    for (const auto& c : cubes) in.cubes.push_back(static_cast<const uint32_t*>(c.data()));
    DeviceScope dev(cfg.cuda_device_id);
    return detail::zonal_table(e, cstats, hist, in, with_counts, out);
}
// The zones of a band of the result as polygons, behind the last finalize on the pipeline's stream: the band as it left the
// pipeline (`out`), in HBM.  Nothing of it runs in finalize: no plane-state event.
Status Pipeline::Impl::polygonize(const std::string& band_name, PolygonSet* out) {
    int b = -1;
    if (Status s = detail::polygonize_check(cfg, out, finalized && zonal_fresh, result.get(), band_name, &b); !s.ok()) return s;
    DeviceScope dev(cfg.cuda_device_id);
    return detail::polygonize_band(bands[(size_t)b].out, cfg.grid, MemoryLocation::Device, stream, out);
}
Status Pipeline::Impl::touched_flags(uint32_t** d, int* tx, int* ty) const {
    return detail::hip_status(pcr_hip_engine_tile_touched(engine, d, tx, ty));
}
// The first Point scatter of a group defines its planes; when this device owns the whole state window (no halo) and
// nobody outside holds pointers into the state, that scatter's tile pass is asked to store the group's finished bands too
// -- finalize after a pipeline's only ingest then has nothing to read back (reference: finalize_result re-reads every
// tile's state, src/engine/pipeline.cpp:1154-1286).
bool Pipeline::Impl::offer_bands(size_t gi) {
    const Group& gr = groups[gi];
    if (gr.select) return false;                   // (its tile pass stores no bands: finalize_select always runs)
    // A group with a filter of its own: the fused tile pass judges "touched" from its OWN scatter's points, the pipeline's
    // flags come from PipelineConfig::filter's survivors -- its bands are made by finalize (the known cost of a spec filter)
    if (gr.cls != 0) return false;
    if (!cfg.finalize_with_first_ingest || gr.defined || gr.glyph.type != GlyphType::Point || state_shared || !result ||
        !d_bands_done.data()) return false;
    if (hg.own_row0 != hg.state_row0 || own_rows() != hg.state_rows || own_rows() <= 0) return false;
    int types[PCR_HIP_MAX_FINALIZE_OUTPUTS];
    float* dsts[PCR_HIP_MAX_FINALIZE_OUTPUTS];
    int n = 0;
    uint32_t own = 0;                              // planes whose own reduction is an output: they can stay in its band
    for (size_t r = 0; r < outputs.size(); ++r) {
        if (outputs[r].group != (int)gi) continue;
        if (n == PCR_HIP_MAX_FINALIZE_OUTPUTS) return false;
        types[n] = static_cast<int>(outputs[r].type);
        dsts[n++] = bands[r].raw;
        if (own_plane(outputs[r].type) >= 0) own |= kPlaneBits[own_plane(outputs[r].type)];
    }
    if (n == 0) return false;
    if (pcr_hip_engine_finalize_with_scatter(engine, n, types, dsts, static_cast<uint32_t*>(d_bands_done.data()) + gi) != PCR_HIP_OK)
        return false;
    return pcr_hip_engine_defer_planes(engine, own & gr.mask) == PCR_HIP_OK;
}

// ---- plane state ---------------------------------------------------------------------------------------------------------
// Six pieces of state say who may trust a group's planes, the touched flags and the bands a scatter stored: Group::fresh,
// defined, bands_with_scatter, planes_in_bands, Impl::state_shared and the device's done words (d_bands_done).  The rule:
//   * a group's planes hold values only once `defined`; until then a scatter defines them itself and every other reader
//     fills the identity first (define_identity);
//   * bands stored by the defining scatter (bands_with_scatter, confirmed by the group's done word) stay good only while
//     nothing else writes the planes or the touched flags: every such writer calls bands_stale() first;
//   * planes left in those bands (planes_in_bands) go back (restore_planes) in front of everything that reads or writes the
//     planes or the flags, finalize apart;
//   * once a plane or flag pointer has left the pipeline (state_shared) no scatter is offered bands again.
// Every assignment to that state is in this block: two primitives (restore_planes, bands_stale), the identity fill, and one
// method per event -- a scatter about to write the planes (bands_stale + scatter_mode), a scatter finished (scatter_done),
// state imported from outside (bands_stale + state_imported), plane pointers leaving (planes_leave), the writable flag
// pointer leaving (flags_leave), the host learning a done word is 0 (done_word_is_zero).

// Enqueues the rebuild of the planes a group's defining scatter left in its bands and clears the mask.  The kernel is
// conditional on the group's done word (0: the scatter stored the planes after all), so no host wait is needed.
Status Pipeline::Impl::restore_planes(size_t gi, bool* enqueued) {
    Group& gr = groups[gi];
    const uint32_t m = gr.planes_in_bands;
    if (!m) return Status::success();
    gr.planes_in_bands = 0;
    const float* src[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t r = 0; r < outputs.size(); ++r) {
        const int p = outputs[r].group == (int)gi ? own_plane(outputs[r].type) : -1;
        if (p >= 0 && (m & kPlaneBits[p])) src[p] = bands[r].raw;
    }
    uint32_t* d_touched = nullptr;
    Status s = touched_flags(&d_touched);
    if (!s.ok()) return s;
    if (enqueued) *enqueued = true;
    return detail::hip_status(pcr_hip_planes_from_bands_if(&hg, &gr.view, m, src, d_touched,
                                                           static_cast<const uint32_t*>(d_bands_done.data()) + gi, stream));
}
Status Pipeline::Impl::restore_all_planes(bool* enqueued) {
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        Status s = restore_planes(gi, enqueued);
        if (!s.ok()) return s;
    }
    return Status::success();
}
// Bands a scatter may have stored are stale as soon as anything else writes the planes or the touched flags.
// Planes those bands still hold are put back FIRST, while the flags and the bands are what the scatter left.
Status Pipeline::Impl::bands_stale() {
    Status s = restore_all_planes();
    for (auto& gr : groups) gr.bands_with_scatter = false;
    return s;
}
// Identity values into a group's planes where nothing has defined them yet.  (finalize's form: it reads the planes of a
// group only where the done word says they were stored)
Status Pipeline::Impl::define_identity(Group& gr) {
    if (gr.defined) return Status::success();
    const int64_t cells = (int64_t)hg.state_rows * hg.width;
    if (gr.select) {                                 // the identity of the packed words is 0
        Status s = detail::hip_status(pcr_hip_memset(gr.packed.data(), 0, (size_t)cells * sizeof(uint64_t), stream));
        if (!s.ok()) return s;
        gr.defined = true;
        return Status::success();
    }
    for (int p = 0; p < 4; ++p) {
        if (!(gr.mask & kPlaneBits[p])) continue;
        Status s = detail::hip_status(pcr_hip_plane_fill(static_cast<float*>(gr.planes[p].data()), detail::plane_identity(false, p), cells, stream));
        if (!s.ok()) return s;
    }
    gr.defined = true;
    return Status::success();
}
// The same for every reader that may come before the group's first scatter (finalize of an empty pipeline, checkpoints,
// the halo exchange of a rank without points, state_planes()).
// Planes the defining scatter left in its bands are put back as well (restore_planes): what this returns from can be read.
Status Pipeline::Impl::define_planes(Group& gr) {
    Status s = define_identity(gr);
    return s.ok() ? restore_planes((size_t)(&gr - groups.data())) : s;
}
Status Pipeline::Impl::define_all_planes() {
    for (auto& gr : groups) {
        Status s = define_planes(gr);
        if (!s.ok()) return s;
    }
    return Status::success();
}
// Event: a scatter is about to write a group's planes (after bands_stale()).  What it is told about them -- 2: the planes
// are still undefined -- the scatter defines every cell of the state window itself (the binned Point path at no extra pass,
// every other path by filling first); 1: identity-filled, nothing accumulated yet
int Pipeline::Impl::scatter_mode(const Group& gr) const {
    return !gr.defined ? 2 : (gr.fresh && gr.glyph.type == GlyphType::Point ? 1 : 0);
}
// Event: that scatter finished.  offered: it was a Point scatter asked to store the group's bands too (offer_bands).
void Pipeline::Impl::scatter_done(Group& gr, bool offered, bool ok) {
    gr.fresh = false;
    gr.bands_with_scatter = offered && ok && pcr_hip_engine_finalize_taken(engine) == 1;
    gr.planes_in_bands = gr.bands_with_scatter ? (uint32_t)pcr_hip_engine_planes_deferred(engine) : 0u;
    if (ok) gr.defined = true;           // (n > 0 here: the scatter ran)
}
// Event: a group's state was copied in from outside (import_window, after bands_stale()).
void Pipeline::Impl::state_imported(Group& gr) {
    gr.defined = true;
    gr.fresh = false;
}
// Event: mutable plane pointers leave the pipeline (state_planes()).
void Pipeline::Impl::planes_leave() {
    {
        DeviceScope dev(cfg.cuda_device_id);
        bool filled = false;
        for (const auto& g : groups) filled = filled || !g.defined || g.planes_in_bands != 0;
        (void)define_all_planes();                      // the caller reads (and may write) them: identity where nothing was ingested
        // The fills run on the pipeline's stream and the caller may read on any other (torch's current stream, a host copy):
        // they are complete when the pointers leave.  Planes that were already defined cost no synchronisation.
        // A MostRecent group leaves as a SNAPSHOT of its two float planes (value in the SUM slot, timestamp in the WGT slot --
        // the layout of its `.pcrt` files, so a sharded save_state gathers it like an Average group), unpacked from the packed
        // words at every call: read-only (the words stay the state), reach 0 (a Point glyph: no part in the halo exchange).
        for (auto& g : groups)
            if (g.select) { (void)unpack_select(g); filled = true; }
        if (filled) (void)pcr_hip_stream_synchronize(stream);
    }
    for (auto& g : groups) g.fresh = false;             // mutable pointers leave the pipeline: assume the planes get written
    state_shared = true;
    (void)bands_stale();                                // (no plane is left in a band: define_all_planes above)
}
// Event: the writable touched-flag pointer leaves the pipeline (the flags may be written from outside: the shard exchange does).
void Pipeline::Impl::flags_leave() {
    state_shared = true;
    // planes a scatter left in its bands are rebuilt from the flags as they are now, and on this pipeline's stream: done
    // before the pointer leaves
    DeviceScope dev(cfg.cuda_device_id);
    bool enqueued = false;
    (void)restore_all_planes(&enqueued);
    if (enqueued) (void)pcr_hip_stream_synchronize(stream);
    (void)bands_stale();
}
// Event: the blocking finalize read a group's done word after its synchronise and found 0 (the scatter stored every plane).
void Pipeline::Impl::done_word_is_zero(Group& gr) { gr.planes_in_bands = 0; }

// ---- the shard accessors: where the events above happen --------------------------------------------------------------------
std::vector<Pipeline::PlaneView> Pipeline::Impl::state_planes() {
    planes_leave();
    std::vector<PlaneView> out;
    for (size_t g = 0; g < groups.size(); ++g)
        for (int p = 0; p < 4; ++p)
            if (groups[g].mask & kPlaneBits[p])
                out.push_back({groups[g].planes[p].data(), (int)kPlaneBits[p], (int)g, groups[g].glyph.type == GlyphType::Point ? 0 : halo});
    return out;
}

std::vector<int> Pipeline::Impl::reduction_groups() const {
    std::vector<int> out;
    for (const auto& o : outputs)
        if (o.group >= 0) out.push_back(o.group);
    return out;
}

void* Pipeline::Impl::tile_touched_device(int* tiles_x, int* tiles_y) {
    uint32_t* d = nullptr;
    int32_t tx = 0, ty = 0;
    if (!touched_flags(&d, &tx, &ty).ok()) return nullptr;
    flags_leave();
    if (tiles_x) *tiles_x = tx;
    if (tiles_y) *tiles_y = ty;
    return d;
}

const void* Pipeline::Impl::tile_touched_device_readonly(int* tiles_x, int* tiles_y) const {
    uint32_t* d = nullptr;
    int32_t tx = 0, ty = 0;
    if (!touched_flags(&d, &tx, &ty).ok()) return nullptr;
    if (tiles_x) *tiles_x = tx;
    if (tiles_y) *tiles_y = ty;
    return d;
}

Status Pipeline::Impl::merge_touched(const void* d_union) {
    if (!d_union) return Status::error(StatusCode::InvalidArgument, "pipeline: merge_touched: null flags");
    DeviceScope dev(cfg.cuda_device_id);
    uint32_t* d = nullptr;
    int32_t tx = 0, ty = 0;
    Status s = touched_flags(&d, &tx, &ty);
    if (!s.ok()) return s;
    // planes still in the bands go back first: a flag that changes clears the done words, and with them what says where they are
    if (!(s = restore_all_planes()).ok()) return s;
    // (the stored bands' device words decide: the host keeps offering them to finalize, whose kernel runs when they are 0)
    // only a flag of a tile this device owns rows of can change its bands (the union used to drop the stored
    // bands whenever ANY tile of the grid changed, i.e. always, on shards that do not share every tile)
    const int th = cfg.grid.tile_height;
    const int t0 = hg.own_row0 / th, t1 = std::min(ty, (hg.own_row1 + th - 1) / th);
    return detail::hip_status(pcr_hip_touched_union_owned(d, static_cast<const uint32_t*>(d_union), tx, ty, std::min(t0, t1), t1,
                                                          static_cast<uint32_t*>(d_bands_done.data()), (int32_t)groups.size(), stream));
}

const float* Pipeline::Impl::result_band_device(int band) {
    if (!finalized || !result || band < 0 || band >= (int)bands.size()) return nullptr;
    return bands[(size_t)band].out;
}

Status Pipeline::Impl::synchronize() { return detail::hip_status(pcr_hip_stream_synchronize(stream)); }

void Pipeline::Impl::profile_enable(bool on, const std::string& only_kernel) {
    pcr_hip_engine_profile_only(engine, only_kernel.c_str());
    pcr_hip_engine_profile_enable(engine, on ? 1 : 0);
}

std::vector<Pipeline::KernelTime> Pipeline::Impl::profile_read(bool reset) {
    std::vector<KernelTime> out;
    pcr_hip_kernel_time buf[32];
    int n = 0;
    if (pcr_hip_engine_profile_read(engine, buf, 32, &n, reset ? 1 : 0) != PCR_HIP_OK) return out;
    for (int i = 0; i < std::min(n, 32); ++i) out.push_back({buf[i].name, buf[i].launches, buf[i].total_ms});
    return out;
}

Pipeline::ScatterInfo Pipeline::Impl::last_scatter() const {
    pcr_hip_scatter_stats st{};
    pcr_hip_engine_stats(engine, &st);
    int fused = 0, deferred = 0;
    for (const auto& g : groups) {
        fused += g.bands_with_scatter ? 1 : 0;
        deferred |= (int)g.planes_in_bands;
    }
    return {st.path, st.lds_tile_w, st.lds_tile_h, st.lds_apron, st.num_bins,
            (size_t)st.points_in, (size_t)st.points_valid, st.scatter_chunk, fused, deferred};
}

// A MostRecent group's float-plane view (slot 0 value, slot 1 timestamp), filled from the packed words: what leaves the
// pipeline (checkpoints, parked bands, state_planes()).  pack_select is the way back.  drop_select_views frees the view
// once the stream is done with it: between two such calls the group costs its 8 bytes per cell only.
Status Pipeline::Impl::unpack_select(Group& gr) {
    if (!gr.select) return Status::success();
    const int64_t cells = (int64_t)hg.state_rows * hg.width;
    Status s = define_planes(gr);
    if (!s.ok()) return s;
    if (!(s = alloc_select_views(gr)).ok()) return s;
    return detail::hip_status(pcr_hip_select_unpack(static_cast<const uint64_t*>(gr.packed.data()), static_cast<float*>(gr.planes[0].data()),
                                                    static_cast<float*>(gr.planes[1].data()), cells, stream));
}
Status Pipeline::Impl::alloc_select_views(Group& gr) {
    const int64_t cells = (int64_t)hg.state_rows * hg.width;
    for (int p = 0; p < 2; ++p) {
        if (gr.planes[p].data()) continue;
        Status s = gr.planes[p].allocate((size_t)std::max<int64_t>(cells, 1) * sizeof(float), MemoryLocation::Device);
        if (!s.ok()) return s;
    }
    return Status::success();
}
Status Pipeline::Impl::pack_select(Group& gr) {
    if (!gr.select) return Status::success();
    const int64_t cells = (int64_t)hg.state_rows * hg.width;
    return detail::hip_status(pcr_hip_select_pack(static_cast<const float*>(gr.planes[0].data()), static_cast<const float*>(gr.planes[1].data()),
                                                  static_cast<uint64_t*>(gr.packed.data()), cells, stream));
}
void Pipeline::Impl::drop_select_views() {                           // (call with the stream synchronized)
    for (auto& gr : groups)
        if (gr.select) { gr.planes[0].release(); gr.planes[1].release(); }
}

// rows a glyph can reach above/below its centre row (sizes the halo of a row-block shard)
int Pipeline::Impl::reach_rows(const GlyphSpec& gl) const {
    double cap = std::min<double>(std::max(0.0f, gl.max_radius_cells), 1 << 20);
    if (gl.type == GlyphType::Gaussian) return (int)std::ceil(cap);
    if (gl.type == GlyphType::Line) {
        double hy = std::fabs((double)gl.default_half_length / cfg.grid.cell_size_y);
        return (int)std::ceil(std::max(hy, cap)) + 1;
    }
    return 0;
}

// A footprint is clipped to the reference tile of its centre cell (Q4): when the owned block is made of whole
// tile rows nothing can land outside it, whatever the glyph.
bool Pipeline::Impl::block_is_whole_tiles() const {
    const int th = cfg.grid.tile_height;
    return hg.own_row0 % th == 0 && (hg.own_row1 % th == 0 || hg.own_row1 == hg.height);
}

// Row-block shards: a Line glyph with a per-point half_length channel reaches |hl_i / cell_size_y| rows (+1 for
// the rounding of the end points), and on north-up grids max_radius_cells does not cap that (hy < 0 passes
// std::min(h, cap) untouched, glyph_kernels.cu:228-234).  Cells beyond the halo would be clipped by the state
// window and never reach their owner: refuse instead of returning a grid that differs from the unsharded one.
// rows_needed: the reach of the longest segment among the points the filter keeps (0: the check does not apply).
Status Pipeline::Impl::line_reach_rows(const GlyphSpec& gl, const void* d_half_length, const uint8_t* d_mask, size_t n, int* rows_needed) {
    *rows_needed = 0;
    if (gl.type != GlyphType::Line || !d_half_length) return Status::success();
    if (own_rows() == hg.height || block_is_whole_tiles()) return Status::success();
    detail::Buffer* word = nullptr;                              // the reduction's device words, kept for the pipeline's life
    Status s = staging_at_least("line_reach:word", 8, &word);
    if (!s.ok()) return s;
    // hy = half_length / cell_size_y goes through std::min(hy, cap) (glyph_kernels.cu:228-234): the sign of half_length
    // that makes hy positive is capped by max_radius_cells, the other one reaches |half_length / cell_size_y| rows
    float max_pos = 0.f, max_neg = 0.f;
    s = detail::hip_status(pcr_hip_signed_max_f32_masked(static_cast<const float*>(d_half_length), d_mask, n,
                                                         static_cast<uint32_t*>(word->data()), &max_pos, &max_neg, stream));
    if (!s.ok()) return s;
    const double acsy = std::fabs(cfg.grid.cell_size_y);
    const float capped_side = cfg.grid.cell_size_y > 0 ? max_pos : max_neg;
    const float free_side = cfg.grid.cell_size_y > 0 ? max_neg : max_pos;
    double rows = std::max(std::ceil((double)free_side / acsy),
                           std::min(std::ceil((double)capped_side / acsy), std::ceil((double)std::max(gl.max_radius_cells, 0.0f))));
    rows += 1.0;                                                 // rounding of the end points
    rows = std::min<double>(rows, cfg.grid.tile_height - 1);
    *rows_needed = (int)rows;
    return Status::success();
}

Status Pipeline::Impl::reach_error(int rows) const {
    return Status::error(StatusCode::InvalidArgument,
        "pipeline: a Line segment of this cloud reaches " + std::to_string((long long)rows) +
        " rows beyond its centre row, but this row-block shard keeps a halo of " + std::to_string(halo) +
        " rows (sized from default_half_length / max_radius_cells); set PipelineConfig.shard_halo_rows >= " +
        std::to_string((long long)rows) + " on every rank, or use tile-aligned row blocks");
}

// The staging buffer `key`, at least `bytes` large: the one way such a buffer grows.  One that is large enough costs nothing and
// waits for nothing; one that has to grow is replaced, with an eighth of slack, once the stream is done with the old block
// (chunks of ingest_async / ingest_file still in flight may read it).
Status Pipeline::Impl::staging_at_least(const std::string& key, size_t bytes, detail::Buffer** out) {
    detail::Buffer& b = staging[key];
    *out = &b;
    if (b.bytes() >= bytes) return Status::success();
    if (b.data()) {
        Status s = detail::hip_status(pcr_hip_stream_synchronize(stream));
        if (!s.ok()) return s;
    }
    return b.allocate(bytes + bytes / 8, MemoryLocation::Device);
}

// Device pointer of a named array of the cloud; host-resident arrays are staged to HBM.
Status Pipeline::Impl::device_array(const void* src, MemoryLocation loc, size_t bytes, const std::string& key, const void** out) {
    if (loc == MemoryLocation::Device) { *out = src; return Status::success(); }
    detail::Buffer* b = nullptr;
    Status s = staging_at_least(key, bytes, &b);
    if (s.ok()) s = detail::hip_status(pcr_hip_memcpy_h2d(b->data(), src, bytes, stream));
    if (s.ok()) *out = b->data();
    return s;
}

// Rows the Line groups of this pipeline need beyond a centre row for THIS cloud (0 when no check applies): what
// ingest() would refuse above the shard's halo.  A sharded caller reduces it over the ranks (MAX) first, so that
// every rank refuses together instead of one rank raising while the others wait in a collective.  The filter is
// not applied here (an upper bound: ingest() itself checks the kept points only).
Status Pipeline::Impl::query_line_reach(const PointCloud& cloud, int* rows_out) {
    *rows_out = 0;
    const size_t n = cloud.count();
    if (n == 0) return Status::success();
    DeviceScope dev(cfg.cuda_device_id);
    for (const auto& gr : groups) {
        if (gr.glyph.type != GlyphType::Line || gr.glyph.half_length_channel.empty()) continue;
        const ChannelDesc* d = cloud.channel(gr.glyph.half_length_channel);
        if (!d || d->dtype != DataType::Float32) continue;
        const void* hl = nullptr;
        Status s = device_array(cloud.channel_data(gr.glyph.half_length_channel), cloud.location(), n * sizeof(float),
                                "ch:" + gr.glyph.half_length_channel, &hl);
        if (!s.ok()) return s;
        int rows = 0;
        if (!(s = line_reach_rows(gr.glyph, hl, nullptr, n, &rows)).ok()) return s;
        *rows_out = std::max(*rows_out, rows);
    }
    return Status::success();
}

// A Line / Gaussian GlyphSpec as the C-ABI takes it: the defaults, and the per-point channels the cloud has (null: the default).
Status Pipeline::Impl::marshal_glyph(const GlyphSpec& gl, const detail::ChannelLookup& channel, pcr_hip_glyph* out) const {
    *out = pcr_hip_glyph{};
    out->type = static_cast<int32_t>(gl.type);
    out->default_direction = gl.default_direction;
    out->default_half_length = gl.default_half_length;
    out->default_sigma_x = gl.default_sigma_x;
    out->default_sigma_y = gl.default_sigma_y;
    out->default_rotation = gl.default_rotation;
    out->max_radius_cells = gl.max_radius_cells;
    Status s = channel(gl.direction_channel, &out->d_direction);
    if (s.ok()) s = channel(gl.half_length_channel, &out->d_half_length);
    if (s.ok()) s = channel(gl.sigma_x_channel, &out->d_sigma_x);
    if (s.ok()) s = channel(gl.sigma_y_channel, &out->d_sigma_y);
    if (s.ok()) s = channel(gl.rotation_channel, &out->d_rotation);
    return s;
}

// PipelineConfig::surface_channels: the band and its geometry into HBM the pipeline owns.  Chunks in flight may still read the
// old band: the stream is waited for first (store_surface waits for the copy, so the caller's grid is free on return).
Status Pipeline::Impl::set_surface(const std::string& name, const Grid& grid, int band) {
    int index = -1;
    pcr_hip_grid geom{};
    Status s = detail::check_surface(cfg, name, grid, band, &index, &geom);
    if (!s.ok()) return s;
    DeviceScope dev(cfg.cuda_device_id);
    if (!(s = detail::hip_status(pcr_hip_stream_synchronize(stream))).ok()) return s;
    return detail::store_surface(grid, band, geom, MemoryLocation::Device, stream, &surfaces[(size_t)index]);
}

// PipelineConfig::polygon_channels: the index built on the host, its tables into HBM the pipeline owns.  Chunks in flight may
// still read the old tables: the stream is waited for first (the upload waits for its copies, so the caller's set is free on
// return).
Status Pipeline::Impl::set_polygons(const std::string& name, const PolygonSet& polygons, const PointInPolygonOptions& options) {
    if (detail::polygon_channel_index(cfg, name) < 0)
        return detail::store_polygons(cfg, name, polygons, options, true, stream, &polygon_sets);        // (the refusal)
    DeviceScope dev(cfg.cuda_device_id);
    Status s = detail::hip_status(pcr_hip_stream_synchronize(stream));
    return s.ok() ? detail::store_polygons(cfg, name, polygons, options, true, stream, &polygon_sets) : s;
}

// ---- ingest: the steps, in the order ingest() takes them ---------------------------------------------------------------------
// Device pointer of a named Float32 channel (Ingest::channel): a surface channel as sample_surfaces left it, a channel of the
// cloud staged once; null for no name or no such channel (-> the GlyphSpec's default).
Status Pipeline::Impl::channel_of(Ingest& in, const std::string& name, const float** out) {
    *out = nullptr;
    if (name.empty()) return Status::success();
    auto hit = in.staged.find(name);
    if (hit != in.staged.end()) { *out = hit->second; return Status::success(); }
    const ChannelDesc* d = in.cloud.channel(name);
    if (!d || d->dtype != DataType::Float32) return Status::success();
    const void* p = nullptr;
    Status st = device_array(in.cloud.channel_data(name), in.cloud.location(), in.n * sizeof(float), "ch:" + name, &p);
    if (st.ok()) in.staged[name] = *out = static_cast<const float*>(p);
    return st;
}

// x and y on the device.  A cloud in another CRS than the grid's: transformed into a staging buffer of their own (the caller's
// device arrays are only read), which every kernel below reads instead.
Status Pipeline::Impl::stage_xy(Ingest& in, const detail::Reprojection& rp) {
    const MemoryLocation loc = in.cloud.location();
    Status s = device_array(in.cloud.x(), loc, in.n * sizeof(double), "x", &in.dx);
    if (s.ok()) s = device_array(in.cloud.y(), loc, in.n * sizeof(double), "y", &in.dy);
    if (!s.ok() || !rp.needed) return s;
    detail::Buffer* rb = nullptr;
    if (!(s = staging_at_least("reproject:xy", 2 * in.n * sizeof(double), &rb)).ok()) return s;
    double* rx = static_cast<double*>(rb->data());
    double* ry = rx + rb->bytes() / (2 * sizeof(double));
    s = detail::hip_status(pcr_hip_transform_xy(&rp.src, &rp.dst, static_cast<const double*>(in.dx),
                                                static_cast<const double*>(in.dy), rx, ry, in.n, stream));
    in.dx = rx;
    in.dy = ry;
    return s;
}

// Surface channels: each gathered once, for all n points, from its band in HBM at the (reprojected) coordinates, into a
// staging buffer of its own that the lookup then answers with -- the filters, the glyph marshalling, the Line reach check and
// every scatter pick it up like a channel the cloud brought.  On the pipeline's stream, no host wait.
Status Pipeline::Impl::sample_surfaces(Ingest& in) {
    for (size_t k = 0; k < surfaces.size(); ++k) {
        const SurfaceChannelConfig& sc = cfg.surface_channels[k];
        const float* dz = nullptr;
        Status s = in.channel(sc.value_channel, &dz);
        if (!s.ok()) return s;
        detail::Buffer* sb = nullptr;
        if (!(s = staging_at_least("surface:" + sc.name, in.n * sizeof(float), &sb)).ok()) return s;
        const detail::Surface& sf = surfaces[k];
        s = detail::hip_status(pcr_hip_sample_grid(&sf.geom, static_cast<const float*>(sf.band.data()), sf.geom.width,
                                                   static_cast<const double*>(in.dx), static_cast<const double*>(in.dy), dz, in.n,
                                                   (int)sc.mode, static_cast<float*>(sb->data()), stream));
        if (!s.ok()) return s;
        in.staged[sc.name] = static_cast<const float*>(sb->data());
    }
    return Status::success();
}

// Polygon channels: each derived once, for all n points, from its index tables in HBM at the (reprojected) coordinates, into a
// staging buffer of its own that the lookup then answers with, like a surface channel.  On the pipeline's stream, no host wait.
Status Pipeline::Impl::locate_polygons(Ingest& in) {
    for (size_t k = 0; k < polygon_sets.size(); ++k) {
        const std::string& name = cfg.polygon_channels[k].name;
        detail::Buffer* pb = nullptr;
        Status s = staging_at_least("polygon:" + name, in.n * sizeof(float), &pb);
        if (s.ok())
            s = polygon_sets[k]->locate(static_cast<const double*>(in.dx), static_cast<const double*>(in.dy), in.n,
                                        static_cast<float*>(pb->data()), true, stream, 1);
        if (!s.ok()) return s;
        in.staged[name] = static_cast<const float*>(pb->data());
    }
    return Status::success();
}

// Filter stage, on the device: one byte mask per filter class, evaluated once per ingest (detail::sweep_filter_classes) and
// honoured by every routing kernel.  Class 0 is PipelineConfig::filter alone; every group scatters under the mask of its
// class.  (The reference gathers values by filter index but routes the UNFILTERED cloud, pipeline.cpp:436-438 vs :662,
// which is why its own WithFilter test is disabled; here a filtered-out point simply does not exist for any reduction.)
Status Pipeline::Impl::filter_stage(Ingest& in) {
    detail::Buffer* mb = nullptr;
    Status s = staging_at_least("filter:mask", detail::filter_stage_bytes(filters, in.n), &mb);
    return s.ok() ? detail::sweep_filter_classes(filters, in.channel, in.n, mb->data(), stream, &in.class_mask, &in.kept) : s;
}

// Row-block shards: every Line group's reach is checked BEFORE the first scatter of this ingest, so a refused
// cloud leaves no group half-accumulated (and, sharded, every rank can agree on the verdict first:
// Pipeline::line_reach_rows + pcr.distributed.ShardedPipeline.ingest).
Status Pipeline::Impl::check_line_reach(Ingest& in) {
    int reach_needed = 0;
    for (const auto& gr : groups) {
        if (gr.glyph.type != GlyphType::Line) continue;
        const float* hl = nullptr;
        Status s = in.channel(gr.glyph.half_length_channel, &hl);
        if (!s.ok()) return s;
        int rows = 0;
        if (!(s = line_reach_rows(gr.glyph, hl, in.class_mask[(size_t)gr.cls], in.n, &rows)).ok()) return s;
        reach_needed = std::max(reach_needed, rows);
    }
    return reach_needed > halo ? reach_error(reach_needed) : Status::success();
}

// One scatter per group, under the mask of its class.
Status Pipeline::Impl::scatter_groups(Ingest& in) {
    const double* dx = static_cast<const double*>(in.dx);
    const double* dy = static_cast<const double*>(in.dy);
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        Group& gr = groups[gi];
        const float* dv = nullptr;
        Status s = in.channel(gr.value_channel, &dv);
        if (!s.ok()) return s;
        pcr_hip_engine_set_point_mask(engine, in.class_mask[(size_t)gr.cls]);
        pcr_hip_engine_planes_fresh(engine, scatter_mode(gr));
        bool offered = false;
        if (gr.select) {                             // (Point glyph: validate_cloud refused anything else)
            const float* dk = nullptr;
            if (!(s = in.channel(gr.key_channel, &dk)).ok()) return s;
            s = detail::hip_status(pcr_hip_scatter_select(engine, static_cast<uint64_t*>(gr.packed.data()), dx, dy, dv, dk, in.n));
        } else if (gr.glyph.type == GlyphType::Point) {
            offered = offer_bands(gi);
            s = detail::hip_status(pcr_hip_scatter_point(engine, gr.mask, &gr.view, dx, dy, dv, in.n));
        } else {
            pcr_hip_glyph hgph{};
            if (!(s = marshal_glyph(gr.glyph, in.channel, &hgph)).ok()) return s;
            s = detail::hip_status(pcr_hip_scatter_glyph(engine, &hgph, gr.mask & (PCR_HIP_PLANE_SUM | PCR_HIP_PLANE_WGT), &gr.view,
                                                         dx, dy, dv, in.n));
        }
        scatter_done(gr, offered, s.ok());
        if (!s.ok()) return s;
    }
    return Status::success();
}

// PipelineConfig::histograms: each cube counts the points its class keeps.  The touched flags it sets are among those the
// scatters (or the touch pass) set already: no band a scatter stored goes stale, no plane is read or written.
Status Pipeline::Impl::scatter_histograms(Ingest& in) {
    for (size_t h = 0; h < hist.entries.size(); ++h) {
        const detail::HistogramEntry& e = hist.entries[h];
        const float* dv = nullptr;
        Status s = in.channel(e.value_channel, &dv);
        if (!s.ok()) return s;
        pcr_hip_engine_set_point_mask(engine, in.class_mask[(size_t)e.cls]);
        s = detail::hip_status(pcr_hip_scatter_histogram(engine, static_cast<uint32_t*>(cubes[h].data()), e.bins, e.lo, e.inv_w,
                                                         static_cast<const double*>(in.dx), static_cast<const double*>(in.dy), dv, in.n));
        if (!s.ok()) return s;
    }
    return Status::success();
}

// PipelineConfig::extremes: each entry's key planes take the points its class keeps, under the same argument about the flags.
Status Pipeline::Impl::scatter_extremes(Ingest& in) {
    for (size_t x = 0; x < ext.entries.size(); ++x) {
        const detail::ExtremesEntry& e = ext.entries[x];
        const float* dv = nullptr;
        Status s = in.channel(e.value_channel, &dv);
        if (!s.ok()) return s;
        pcr_hip_engine_set_point_mask(engine, in.class_mask[(size_t)e.cls]);
        s = detail::hip_status(pcr_hip_scatter_extremes(engine, static_cast<uint32_t*>(ext_keys[x].data()), e.k, e.side,
                                                        static_cast<const double*>(in.dx), static_cast<const double*>(in.dy), dv, in.n));
        if (!s.ok()) return s;
    }
    return Status::success();
}

// PipelineConfig::cell_stats: each entry's three planes take the points its class keeps, likewise.
Status Pipeline::Impl::scatter_cell_stats(Ingest& in) {
    for (size_t x = 0; x < cstats.entries.size(); ++x) {
        const detail::CellStatsEntry& e = cstats.entries[x];
        const float* dv = nullptr;
        Status s = in.channel(e.value_channel, &dv);
        if (!s.ok()) return s;
        pcr_hip_engine_set_point_mask(engine, in.class_mask[(size_t)e.cls]);
        s = detail::hip_status(pcr_hip_scatter_cell_stats(engine, static_cast<uint32_t*>(stat_planes[x].n.data()),
                                                          static_cast<long long*>(stat_planes[x].s1.data()),
                                                          static_cast<unsigned long long*>(stat_planes[x].s2.data()), e.origin, e.inv_res,
                                                          static_cast<const double*>(in.dx), static_cast<const double*>(in.dy), dv, in.n));
        if (!s.ok()) return s;
    }
    return Status::success();
}

// PipelineConfig::point_zonal: every entry's specs folded by its label channel, on the pipeline's stream under the class masks of
// the filter stage.  No coordinate is read, no plane, flag or band touched: no part in the plane-state rules.
Status Pipeline::Impl::fold_point_zonal(Ingest& in) {
    if (!pz_plan.on()) return Status::success();
    detail::PointZonalInputs pin;
    pin.device = true;
    pin.stream = stream;
    pin.n = in.n;
    pin.channel = in.channel;
    pin.mask = [&in](int cls) { return in.class_mask[(size_t)cls]; };
    return detail::point_zonal_fold(pz_plan, pz_state, pin);
}

// Entry i's rows, made in HBM behind everything on the pipeline's stream.
Status Pipeline::Impl::point_zonal(int i, PointZonalTable* out, bool with_counts) {
    if (!out || i < 0 || (size_t)i >= pz_plan.entries.size())
        return Status::error(StatusCode::InvalidArgument, "pipeline: point_zonal: no point_zonal entry " + std::to_string(i));
    DeviceScope dev(cfg.cuda_device_id);
    return detail::point_zonal_table(pz_plan.entries[(size_t)i], pz_state.tables[(size_t)i], stream, with_counts, out);
}

Status Pipeline::Impl::ingest(const PointCloud& cloud, bool wait) {
    Ingest in{cloud, cloud.count()};
    if (in.n == 0) return Status::success();
    DeviceScope dev(cfg.cuda_device_id);
    // validate every predicate and reduction before touching state (pipeline_common.cpp: the reference's checks and messages)
    Status s = surfaces.empty() ? Status::success() : detail::validate_surfaces(cfg, cloud, surfaces);
    if (s.ok() && !polygon_sets.empty()) s = detail::validate_polygon_channels(cfg, cloud, polygon_sets);
    if (s.ok()) s = detail::validate_cloud(cfg, cloud, PCR_HIP_MAX_FILTER_SET, PCR_HIP_MAX_FILTER_PREDICATES);
    if (s.ok() && pz_plan.on()) s = detail::validate_point_zonal(cfg, cloud);
    detail::Reprojection rp;
    if (s.ok()) s = detail::plan_reprojection(cfg, cloud, &rp);
    if (!s.ok()) return s;
    in.channel = [this, &in](const std::string& name, const float** out) { return channel_of(in, name, out); };

    if (!(s = stage_xy(in, rp)).ok()) return s;
    if (!(s = sample_surfaces(in)).ok()) return s;
    if (!(s = locate_polygons(in)).ok()) return s;
    if (!(s = filter_stage(in)).ok()) return s;
    if (in.kept == 0) return Status::success();                  // pipeline.cpp:349-353: PipelineConfig::filter keeps nothing
    pcr_hip_engine_set_point_mask(engine, in.class_mask[0]);
    struct MaskGuard {
        pcr_hip_engine* e;
        ~MaskGuard() { pcr_hip_engine_set_point_mask(e, nullptr); }
    } mask_guard{engine};
    if (!(s = check_line_reach(in)).ok()) return s;

    // (this cloud's points change the planes and the touched flags)
    zonal_fresh = false;
    if (!(s = bands_stale()).ok()) return s;
    // The touched flags are PipelineConfig::filter's survivors', whatever the groups' own filters keep.  An unfiltered group's
    // scatter sets exactly those; when every group is filtered a pass of its own does, ahead of the first scatter.
    bool flags_by_scatter = !filters.any();
    for (const auto& gr : groups) flags_by_scatter = flags_by_scatter || gr.cls == 0;
    if (!flags_by_scatter) {
        s = detail::hip_status(pcr_hip_engine_touch(engine, static_cast<const double*>(in.dx), static_cast<const double*>(in.dy), in.n));
        if (!s.ok()) return s;
    }
    if (!(s = scatter_groups(in)).ok()) return s;
    if (!(s = scatter_histograms(in)).ok()) return s;
    if (!(s = scatter_extremes(in)).ok()) return s;
    if (!(s = scatter_cell_stats(in)).ok()) return s;
    if (!(s = fold_point_zonal(in)).ok()) return s;
    // host arrays may be reused by the caller as soon as we return (ingest_async: page-locked arrays are
    // read by the DMA engine later, the caller keeps them alive until synchronize())
    const MemoryLocation loc = cloud.location();
    if (loc != MemoryLocation::Device && (wait || loc != MemoryLocation::HostPinned)) {
        s = detail::hip_status(pcr_hip_stream_synchronize(stream));
        if (!s.ok()) return s;
    }

    points += in.kept;              // points_processed += filtered_count (pipeline.cpp:749)
    collections++;
    if (callback) {
        ProgressInfo info = stats();
        if (!callback(info))
            return Status::error(StatusCode::InvalidArgument, "pipeline: cancelled by user");
    }
    return Status::success();
}

// The result grid, the table of leaving bands and the device buffers behind it are allocated
// once, at create: finalize only launches kernels.
Status Pipeline::Impl::allocate_result() {
    const int rows = own_rows();
    const int W = hg.width;
    std::vector<BandDesc> descs;
    for (const auto& o : outputs) {
        BandDesc b;
        b.name = o.band_name;
        b.dtype = DataType::Float32;
        b.is_state = false;
        descs.push_back(b);
    }
    if (descs.empty()) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate result grid");
    detail::append_ground_bands(ground, descs);
    detail::append_terrain_bands(terrain, descs);
    detail::append_tree_bands(tree_plan, descs);
    if (rows <= 0) { result.reset(); return Status::success(); }
    const bool on_device = cfg.result_location == MemoryLocation::Device;
    result = on_device ? Grid::create(W, rows, descs, MemoryLocation::Device)
                       : Grid::create_host_page_locked(W, rows, descs);
    if (!result) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate result grid");
    if (rows == cfg.grid.height) (void)result->set_geometry(detail::result_geometry(cfg));     // (a shard's block is no grid of its own)
    // the table of leaving bands and the buffers behind it: the rule (device_pipeline.h, LeavingBand) applied once
    const size_t n_out = outputs.size();
    bands.assign(n_out + (size_t)ground.extra_bands() + (size_t)terrain.extra_bands() + (size_t)tree_plan.extra_bands(), LeavingBand{});
    band_buffers.clear();
    Status s = Status::success();
    auto owned = [&]() -> float* {
        if (!s.ok()) return nullptr;
        band_buffers.emplace_back();
        s = band_buffers.back().allocate((size_t)rows * W * sizeof(float), MemoryLocation::Device);
        return static_cast<float*>(band_buffers.back().data());
    };
    for (size_t b = 0; b < bands.size() && s.ok(); ++b) {
        // (behind the outputs only the DTM is filled: without a ground plan band n_out is the first terrain band)
        const bool filled = cfg.fill_nodata_radius > 0 && (b < n_out ? detail::fills_nodata(outputs[b].type) : ground.on && b == n_out);
        float* const grid_band = on_device ? result->band_f32((int)b) : nullptr;
        bands[b].raw = on_device && !filled ? grid_band : owned();
        bands[b].out = !filled ? bands[b].raw : on_device ? grid_band : owned();
    }
    return s;
}

Status Pipeline::Impl::finalize(bool wait) {
    const int rows = own_rows();
    const int W = hg.width;
    if (outputs.empty()) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate result grid");
    if (rows <= 0) return Status::success();
    DeviceScope dev(cfg.cuda_device_id);
    const bool on_device = cfg.result_location == MemoryLocation::Device;
    if (!result) {
        Status as = allocate_result();
        if (!as.ok()) return as;
    }
    for (auto& gr : groups) {                     // a group no cloud ever reached
        Status ds = define_identity(gr);
        if (!ds.ok()) return ds;
    }
    uint32_t* d_touched = nullptr;
    Status s = touched_flags(&d_touched);
    if (!s.ok()) return s;
    // Bands the defining scatter may have stored: whether it did is a word the device wrote (not when the scan split a
    // bin; cleared again by a touched-flag union that changed a flag).  The blocking call is going to wait for the stream
    // anyway: it waits FIRST, reads the word, and enqueues the group's kernel only when the word says the bands are not
    // there -- after a pipeline's only ingest nothing runs behind the tile pass.  finalize_async leaves the decision to
    // the kernel (pcr_hip_finalize_group_unless), which reads the word when it runs.
    bool host_decides = false;
    if (wait)
        for (const auto& gr : groups) host_decides = host_decides || gr.bands_with_scatter;
    if (host_decides) {
        s = detail::hip_status(pcr_hip_stream_synchronize(stream));
        if (!s.ok()) return s;
    }
    bool enqueued = !host_decides;           // anything on the stream since that synchronise
    // one sweep per accumulation group: its planes are read once for all of its bands
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        std::vector<int> types;
        std::vector<float*> dsts;
        std::vector<size_t> bands_of;
        auto flush = [&]() -> Status {
            if (types.empty()) return Status::success();
            // (a group whose bands the defining scatter stored: the kernel returns at once when the device word says so)
            const uint32_t* done = groups[gi].bands_with_scatter ? static_cast<const uint32_t*>(d_bands_done.data()) + gi : nullptr;
            if (done && host_decides) {
                if (*static_cast<const volatile uint32_t*>(done) != 0u) { types.clear(); dsts.clear(); return Status::success(); }
                done = nullptr;              // (known to be 0: the kernel need not read it across the bus)
                done_word_is_zero(groups[gi]);
            }
            enqueued = true;
            Status fs = detail::hip_status(pcr_hip_finalize_group_unless(&hg, &groups[gi].view, d_touched, (int)types.size(),
                                                                         types.data(), dsts.data(), done, stream));
            types.clear();
            dsts.clear();
            return fs;
        };
        for (size_t r = 0; r < outputs.size(); ++r) {
            if (outputs[r].group != (int)gi) continue;
            if (groups[gi].select) {
                s = detail::hip_status(pcr_hip_finalize_select(&hg, static_cast<const uint64_t*>(groups[gi].packed.data()), d_touched,
                                                               bands[r].raw, stream));
                if (!s.ok()) return s;
                enqueued = true;
                bands_of.push_back(r);
                continue;
            }
            types.push_back(static_cast<int>(outputs[r].type));
            dsts.push_back(bands[r].raw);
            bands_of.push_back(r);
            if (types.size() == PCR_HIP_MAX_FINALIZE_OUTPUTS && !(s = flush()).ok()) return s;
        }
        if (!(s = flush()).ok()) return s;
        for (size_t r : bands_of)            // behind the band's finalize kernel (or the scatter that stored it)
            if (!(s = band_leaves(r, &enqueued)).ok()) return s;
    }
    if (!(s = finalize_histograms(&enqueued)).ok()) return s;
    if (!(s = finalize_extremes(&enqueued)).ok()) return s;
    if (!(s = finalize_cell_stats(&enqueued)).ok()) return s;
    if (!(s = finalize_ground(&enqueued)).ok()) return s;
    if (!(s = finalize_terrain(&enqueued)).ok()) return s;
    if (!(s = finalize_trees(&enqueued)).ok()) return s;
    // write_cog: the overview levels are one more pass over the bands where they are, in HBM, behind the finalize
    // kernels on the same stream; only the levels (a third of the data) cross the bus, the host never halves the grid.
    std::vector<std::unique_ptr<Grid>> levels;
    const GeoTiffOptions out_opt = pipeline_output_options(cfg.write_cog);
    if (!cfg.output_path.empty() && out_opt.overviews != 0) {
        const int n = detail::overview_levels(out_opt.overviews, W, rows);
        if (n > 0) {
            std::vector<const float*> dev_bands;
            std::vector<BandDesc> descs;
            for (size_t b = 0; b < bands.size(); ++b) {
                dev_bands.push_back(bands[b].out);
                descs.push_back(result->band_desc((int)b));
            }
            std::vector<std::unique_ptr<Grid>> d_levels;
            s = detail::build_overviews_device(dev_bands, W, rows, descs, n, detail::overview_mode(out_opt.overview_resampling),
                                               stream, d_levels);
            if (!s.ok()) return s;
            enqueued = true;
            for (const auto& d : d_levels) {
                auto h = Grid::create_host_page_locked(d->cols(), d->rows(), descs);
                if (!h) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate the overview levels");
                if (!(s = h->copy_from(*d, stream)).ok()) return s;
                levels.push_back(std::move(h));
            }
            s = detail::hip_status(pcr_hip_stream_synchronize(stream));      // d_levels is released at the end of this block
            if (!s.ok()) return s;
            enqueued = false;
        }
    }
    std::vector<const Grid*> level_ptrs;
    for (const auto& l : levels) level_ptrs.push_back(l.get());
    // finalize_async: a device-resident result is stream-ordered like everything else on the device
    if ((wait || !on_device || !cfg.output_path.empty()) && enqueued) {
        s = detail::hip_status(pcr_hip_stream_synchronize(stream));
        if (!s.ok()) return s;
    }
    finalized = true;
    zonal_fresh = true;
    if (!cfg.output_path.empty()) {
        // pipeline.cpp:1351-1361 of the reference: the finalized grid goes to output_path as GeoTIFF.
        // A shard writes its own row block (georeferenced as such); a device-resident result is copied out first.
        GridConfig out_cfg = cfg.grid;
        if (rows != cfg.grid.height) {
            out_cfg.height = rows;
            out_cfg.bounds.max_y = cfg.grid.bounds.max_y + hg.own_row0 * cfg.grid.cell_size_y;
            out_cfg.bounds.min_y = out_cfg.bounds.max_y + rows * cfg.grid.cell_size_y;
            if (out_cfg.bounds.min_y > out_cfg.bounds.max_y) std::swap(out_cfg.bounds.min_y, out_cfg.bounds.max_y);
        }
        if (on_device) {
            std::unique_ptr<Grid> host = result->to(MemoryLocation::Host);
            if (!host) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to copy the result grid to the host");
            return write_geotiff(cfg.output_path, *host, out_cfg, out_opt, level_ptrs);
        }
        return write_geotiff(cfg.output_path, *result, out_cfg, out_opt, level_ptrs);
    }
    return Status::success();
}

// ---- `.pcrt` checkpoints ---------------------------------------------------------------
// A whole-grid pipeline checkpoints every touched tile.  A row-block shard WRITES the tiles it owns whole -- which is all
// of them when its block is made of whole reference-tile rows (ShardedPipeline(align = tile_height); the N = 2 and 4 blocks
// of C5): every rank writes its own files into the same directory and their union is the pipeline's checkpoint, readable
// by an unsharded pipeline too.  A block that cuts tiles shares them with its neighbours: ShardedPipeline::save_state
// gathers the state to one rank for those.  Any shard LOADS: it takes its own rows out of every tile file they meet.
Status Pipeline::Impl::checkpoint_dir(const std::string& dir_in, std::string* dir, bool writing) const {
    *dir = dir_in.empty() ? cfg.state_dir : dir_in;
    if (dir->empty()) return Status::error(StatusCode::InvalidArgument, "pipeline: no state directory given");
    if (writing && own_rows() != hg.height && !block_is_whole_tiles())
        return Status::error(StatusCode::NotImplemented,
            "pipeline: this row block cuts a reference tile it shares with a neighbour, so no rank can write that tile alone: "
            "ShardedPipeline.save_state gathers the state for it, or shard with align = tile_height");
    return Status::success();
}
detail::StateWindow Pipeline::Impl::state_window(std::vector<std::vector<float>>& planes) const {
    detail::StateWindow w = detail::window_over(planes, hg.state_row0, hg.state_rows);
    w.own_row0 = hg.own_row0;
    w.own_row1 = hg.own_row1;
    return w;
}

Status Pipeline::Impl::export_window(std::vector<std::vector<float>>& planes, std::vector<uint32_t>& touched) {
    DeviceScope dev(cfg.cuda_device_id);
    Status s = define_all_planes();
    if (!s.ok()) return s;
    const size_t cells = (size_t)hg.state_rows * hg.width;
    planes.assign(groups.size() * 4, {});
    for (auto& gr : groups)
        if (!(s = unpack_select(gr)).ok()) return s;
    for (size_t gi = 0; gi < groups.size(); ++gi)
        for (int p = 0; p < 4; ++p) {
            if (!(groups[gi].mask & kPlaneBits[p])) continue;
            planes[gi * 4 + p].resize(cells);
            s = detail::hip_status(pcr_hip_memcpy_d2h(planes[gi * 4 + p].data(), groups[gi].planes[p].data(), cells * sizeof(float), stream));
            if (!s.ok()) return s;
        }
    uint32_t* d_touched = nullptr;
    int tx = 0, ty = 0;
    if (!(s = touched_flags(&d_touched, &tx, &ty)).ok()) return s;
    touched.resize((size_t)tx * ty);
    if (!(s = detail::hip_status(pcr_hip_memcpy_d2h(touched.data(), d_touched, touched.size() * 4, stream))).ok()) return s;
    s = detail::hip_status(pcr_hip_stream_synchronize(stream));
    if (!state_shared) drop_select_views();
    return s;
}
Status Pipeline::Impl::import_window(const std::vector<std::vector<float>>& planes, const std::vector<uint32_t>& touched) {
    DeviceScope dev(cfg.cuda_device_id);
    Status s = bands_stale();
    if (!s.ok()) return s;
    const size_t cells = (size_t)hg.state_rows * hg.width;
    if (planes.size() != groups.size() * 4)
        return Status::error(StatusCode::InvalidArgument, "pipeline: parked state does not match the pipeline's groups");
    for (size_t gi = 0; gi < groups.size(); ++gi) {
        if (groups[gi].select && !(s = alloc_select_views(groups[gi])).ok()) return s;
        for (int p = 0; p < 4; ++p) {
            if (!(groups[gi].mask & kPlaneBits[p])) continue;
            if (planes[gi * 4 + p].size() != cells)
                return Status::error(StatusCode::InvalidArgument, "pipeline: parked state does not match the band's window");
            s = detail::hip_status(pcr_hip_memcpy_h2d(groups[gi].planes[p].data(), planes[gi * 4 + p].data(), cells * sizeof(float), stream));
            if (!s.ok()) return s;
        }
        // (a state that comes from outside is judged by the acceptance rule again: a NaN or <= -FLT_MAX timestamp = empty)
        if (groups[gi].select && !(s = pack_select(groups[gi])).ok()) return s;
        state_imported(groups[gi]);
    }
    uint32_t* d_touched = nullptr;
    int tx = 0, ty = 0;
    if (!(s = touched_flags(&d_touched, &tx, &ty)).ok()) return s;
    if (touched.size() != (size_t)tx * ty)
        return Status::error(StatusCode::InvalidArgument, "pipeline: parked touched flags do not match the tile grid");
    if (!(s = detail::hip_status(pcr_hip_memcpy_h2d(d_touched, touched.data(), touched.size() * 4, stream))).ok()) return s;
    s = detail::hip_status(pcr_hip_stream_synchronize(stream));
    if (!state_shared) drop_select_views();
    return s;
}

Status Pipeline::Impl::save_state(const std::string& dir_in) {
    if (!cfg.histograms.empty()) return detail::histograms_checkpoint_error();
    if (!cfg.extremes.empty()) return detail::extremes_checkpoint_error();
    if (!cfg.cell_stats.empty()) return detail::cell_stats_checkpoint_error();
    if (!cfg.point_zonal.empty()) return detail::point_zonal_checkpoint_error();
    std::string dir;
    Status s = checkpoint_dir(dir_in, &dir, true);
    if (!s.ok()) return s;
    std::vector<std::vector<float>> planes;
    std::vector<uint32_t> touched;
    if (!(s = export_window(planes, touched)).ok()) return s;
    return detail::write_state_tiles(cfg.grid, detail::state_outputs(outputs), state_window(planes), touched, dir);
}

Status Pipeline::Impl::load_state(const std::string& dir_in) {
    if (!cfg.histograms.empty()) return detail::histograms_checkpoint_error();
    if (!cfg.extremes.empty()) return detail::extremes_checkpoint_error();
    if (!cfg.cell_stats.empty()) return detail::cell_stats_checkpoint_error();
    if (!cfg.point_zonal.empty()) return detail::point_zonal_checkpoint_error();
    std::string dir;
    Status s = checkpoint_dir(dir_in, &dir, false);
    if (!s.ok()) return s;
    std::vector<std::vector<float>> planes;
    std::vector<uint32_t> touched;
    if (!(s = export_window(planes, touched)).ok()) return s;          // files overlay the current state
    size_t loaded = 0;
    if (!(s = detail::read_state_tiles(cfg.grid, detail::state_outputs(outputs), state_window(planes), touched, dir, &loaded)).ok()) return s;
    if (!loaded) return Status::success();
    return import_window(planes, touched);                              // (drops bands a scatter stored, marks the planes defined)
}

ProgressInfo Pipeline::Impl::stats() const {
    ProgressInfo info;
    info.collections_processed = collections;
    info.collections_total = 0;
    info.points_processed = points;
    info.tiles_active = 0;
    DeviceScope dev(cfg.cuda_device_id);
    uint32_t* d_touched = nullptr;
    int tx = 0, ty = 0;
    if (engine && touched_flags(&d_touched, &tx, &ty).ok()) {
        std::vector<uint32_t> h((size_t)tx * ty);
        if (pcr_hip_memcpy_d2h(h.data(), d_touched, h.size() * sizeof(uint32_t), stream) == PCR_HIP_OK &&
            pcr_hip_stream_synchronize(stream) == PCR_HIP_OK)
            for (uint32_t v : h) info.tiles_active += v ? 1 : 0;
    }
    info.elapsed_seconds = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
    return info;
}

}  // namespace pcr
