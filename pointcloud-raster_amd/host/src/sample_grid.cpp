// sample_grid.cpp -- pcr/core/sample_grid.h, and the pieces of it the pipelines share (sample_grid.h).  The per-point
// arithmetic is the C-ABI's (csrc/sample_grid.hpp): pcr_hip_sample_grid for a Device cloud, pcr_hip_sample_grid_host otherwise.
#include "sample_grid.h"

#include "pcr/core/point_cloud.h"
#include "pcr/core/reproject.h"

#include <algorithm>

#ifdef _OPENMP
#include <omp.h>
#endif

namespace pcr {
namespace detail {

namespace {
Status refuse(const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: " + msg); }
}  // namespace

Status plan_surfaces(const PipelineConfig& cfg) {
    const auto& list = cfg.surface_channels;
    if (list.empty()) return Status::success();
    if (list.size() > kMaxSurfaceChannels)
        return refuse("more than " + std::to_string(kMaxSurfaceChannels) + " surface_channels (" + std::to_string(list.size()) + " given)");
    for (size_t i = 0; i < list.size(); ++i) {
        const std::string where = "surface_channels[" + std::to_string(i) + "]";
        if (list[i].name.empty()) return refuse(where + ".name is empty");
        for (size_t k = 0; k < i; ++k)
            if (list[k].name == list[i].name) return refuse(where + ".name '" + list[i].name + "' is given twice");
        if (list[i].mode != SampleMode::Nearest && list[i].mode != SampleMode::Bilinear) return refuse(where + ".mode is no sample mode");
    }
    for (size_t i = 0; i < list.size(); ++i)
        if (surface_index(cfg, list[i].value_channel) >= 0)
            return refuse("surface_channels[" + std::to_string(i) + "].value_channel '" + list[i].value_channel +
                          "' is itself a surface channel (surface channels do not chain)");
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0)
        return refuse("surface_channels are not supported on a row-block shard");
    return Status::success();
}

Status surfaces_out_of_core_error() { return refuse("surface_channels are not supported on a pipeline that runs out of core"); }

pcr_hip_grid surface_geom(const GridConfig& g) {
    pcr_hip_grid s{};
    s.min_x = g.bounds.min_x; s.min_y = g.bounds.min_y; s.max_x = g.bounds.max_x; s.max_y = g.bounds.max_y;
    s.cell_size_x = g.cell_size_x; s.cell_size_y = g.cell_size_y;
    s.width = g.width; s.height = g.height;
    s.tile_width = std::max(g.width, 1); s.tile_height = std::max(g.height, 1);
    s.own_row0 = 0; s.own_row1 = g.height;
    s.state_row0 = 0; s.state_rows = g.height;
    return s;
}

Status check_surface(const PipelineConfig& cfg, const std::string& name, const Grid& grid, int band, int* index, pcr_hip_grid* geom) {
    *index = surface_index(cfg, name);
    if (*index < 0) return refuse("set_surface: '" + name + "' names no surface channel of this pipeline");
    const GridConfig* g = grid.geometry();
    if (!g) return refuse("set_surface: the grid carries no geometry (Grid::set_geometry)");
    if (band < 0 || band >= grid.num_bands())
        return refuse("set_surface: band " + std::to_string(band) + " is outside the grid (" + std::to_string(grid.num_bands()) + " bands)");
    if (!grid.band_f32(band)) return refuse("set_surface: band " + std::to_string(band) + " is not Float32");
    const int have = crs_epsg(g->crs), want = crs_epsg(pipeline_crs(cfg));
    if (have != 0 && want != 0 && have != want)
        return Status::error(StatusCode::CrsError, "pipeline: set_surface: the surface is in EPSG:" + std::to_string(have) +
                                                   ", the pipeline's grid in EPSG:" + std::to_string(want) +
                                                   " (the reprojected points are sampled: the surface must be in the grid's CRS)");
    *geom = surface_geom(*g);
    return Status::success();
}

Status store_surface(const Grid& grid, int band, const pcr_hip_grid& geom, MemoryLocation loc, pcr_hip_stream stream, Surface* out) {
    const size_t bytes = (size_t)grid.cell_count() * sizeof(float);
    if (out->band.bytes() != bytes || out->band.location() != loc) {
        Status s = out->band.allocate(bytes, loc);
        if (!s.ok()) { out->set = false; return s; }
    }
    const bool device = loc == MemoryLocation::Device || grid.location() == MemoryLocation::Device;
    Status s = copy_bytes(out->band.data(), loc, grid.band_f32(band), grid.location(), bytes, stream);
    if (s.ok() && device) s = hip_status(pcr_hip_stream_synchronize(stream));      // the caller's grid may die or change now
    out->set = s.ok();
    out->geom = geom;
    return s;
}

Status validate_surfaces(const PipelineConfig& cfg, const PointCloud& cloud, const std::vector<Surface>& surfaces) {
    for (size_t i = 0; i < cfg.surface_channels.size(); ++i) {
        const SurfaceChannelConfig& sc = cfg.surface_channels[i];
        if (i >= surfaces.size() || !surfaces[i].set)
            return refuse("surface channel '" + sc.name + "' has no surface (call set_surface first)");
        if (cloud.has_channel(sc.name))
            return refuse("the cloud already carries a channel named '" + sc.name + "', which this pipeline derives from a surface");
        if (sc.value_channel.empty()) continue;
        const ChannelDesc* d = cloud.channel(sc.value_channel);
        if (!d || !cloud.channel_data(sc.value_channel))
            return refuse("surface channel '" + sc.name + "': value channel not found: " + sc.value_channel);
        if (d->dtype != DataType::Float32) return refuse("surface channel '" + sc.name + "': value channel must be Float32");
    }
    return Status::success();
}

Status sample_host(const pcr_hip_grid& geom, const float* band, int64_t stride, const double* x, const double* y, const float* value,
                   size_t n, SampleMode mode, float* out, int threads) {
    constexpr size_t kChunk = 1 << 16;
    const int64_t chunks = (int64_t)((n + kChunk - 1) / kChunk);
    int rc = PCR_HIP_OK;
#pragma omp parallel for num_threads(std::max(threads, 1)) schedule(static) reduction(max : rc)
    for (int64_t k = 0; k < chunks; ++k) {
        const size_t i0 = (size_t)k * kChunk, m = std::min(kChunk, n - i0);
        rc = std::max(rc, pcr_hip_sample_grid_host(&geom, band, stride, x + i0, y + i0, value ? value + i0 : nullptr, m, (int)mode, out + i0));
    }
    return hip_status(rc);
}

}  // namespace detail

Status sample_grid(PointCloud& cloud, const Grid& surface, int band, const std::string& out_channel, const std::string& value_channel,
                   SampleMode mode) {
    auto refuse = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "sample_grid: " + msg); };
    const GridConfig* g = surface.geometry();
    if (!g) return refuse("the grid carries no geometry (Grid::set_geometry)");
    if (band < 0 || band >= surface.num_bands())
        return refuse("band " + std::to_string(band) + " is outside the grid (" + std::to_string(surface.num_bands()) + " bands)");
    if (!surface.band_f32(band)) return refuse("band " + std::to_string(band) + " is not Float32");
    if (out_channel.empty()) return refuse("the output channel needs a name");
    if (mode != SampleMode::Nearest && mode != SampleMode::Bilinear) return refuse("unknown mode");
    if (!value_channel.empty()) {
        const ChannelDesc* d = cloud.channel(value_channel);
        if (!d) return refuse("value channel not found: " + value_channel);
        if (d->dtype != DataType::Float32) return refuse("value channel must be Float32");
    }
    if (const ChannelDesc* d = cloud.channel(out_channel)) {
        if (d->dtype != DataType::Float32) return refuse("the existing channel '" + out_channel + "' is not Float32");
    }
    const int have = crs_epsg(g->crs), want = crs_epsg(cloud.crs());
    if (have != 0 && want != 0 && have != want)
        return Status::error(StatusCode::CrsError, "sample_grid: the surface is in EPSG:" + std::to_string(have) + ", the cloud in EPSG:" +
                                                   std::to_string(want) + "; reproject the cloud first");
    if (!cloud.has_channel(out_channel)) {
        Status s = cloud.add_channel(out_channel, DataType::Float32);
        if (!s.ok()) return s;
    }
    const size_t n = cloud.count();
    if (n == 0) return Status::success();
    const pcr_hip_grid geom = detail::surface_geom(*g);
    const bool on_device = cloud.location() == MemoryLocation::Device;
    const bool grid_on_device = surface.location() == MemoryLocation::Device;
    const float* band_ptr = surface.band_f32(band);
    detail::Buffer across;                                   // the band on the cloud's side, when it lives on the other
    if (on_device != grid_on_device) {
        const size_t bytes = (size_t)surface.cell_count() * sizeof(float);
        Status s = across.allocate(bytes, on_device ? MemoryLocation::Device : MemoryLocation::Host);
        if (s.ok()) s = detail::copy_bytes(across.data(), across.location(), band_ptr, surface.location(), bytes, nullptr);
        if (s.ok()) s = detail::hip_status(pcr_hip_stream_synchronize(nullptr));
        if (!s.ok()) return s;
        band_ptr = static_cast<const float*>(across.data());
    }
    const float* value = value_channel.empty() ? nullptr : cloud.channel_f32(value_channel);
    float* out = cloud.channel_f32(out_channel);
    if (on_device) {
        Status s = detail::hip_status(pcr_hip_sample_grid(&geom, band_ptr, surface.cols(), cloud.x(), cloud.y(), value, n, (int)mode, out, nullptr));
        return s.ok() ? detail::hip_status(pcr_hip_stream_synchronize(nullptr)) : s;
    }
    int threads = 1;
#ifdef _OPENMP
    threads = omp_get_max_threads();
#endif
    return detail::sample_host(geom, band_ptr, surface.cols(), cloud.x(), cloud.y(), value, n, mode, out, threads);
}

}  // namespace pcr
