// polygons.cpp -- rasterize_polygons: a polygon set burnt into a label grid where the grid is to live (pcr/core/polygons.h).
#include "polygons.h"

#include "pipeline_common.h"

#ifdef _OPENMP
#include <omp.h>
#endif

namespace pcr {
namespace detail {

Status rasterize_into(const PolygonSet& set, const GridConfig& geometry, const RasterizeOptions& options, float* dst,
                      MemoryLocation loc, void* stream) {
    auto refuse = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "rasterize_polygons: " + msg); };
    const int64_t V = set.num_vertices(), R = set.num_rings(), P = set.num_polygons();
    if (set.coords.size() % 2 != 0) return refuse("coords must hold an x and a y for every vertex");
    if (set.ring_offsets.empty() || set.polygon_offsets.empty()) return refuse("null or inconsistent offsets");
    if (P > pcrhip::raster::kMaxPolygons) return refuse("more than 2^31 - 2 polygons");
    if (!set.values.empty() && (int64_t)set.values.size() != P) return refuse("values must be empty or one per polygon");
    const pcr_hip_grid g = to_hip_grid(geometry);
    pcr_hip_rasterize_params p{};
    p.background = options.background;
    const float* values = set.values.empty() ? nullptr : set.values.data();
    if (loc != MemoryLocation::Device)
        return hip_status(pcr_hip_rasterize_polygons_host(&g, set.coords.data(), V, set.ring_offsets.data(), R, set.polygon_offsets.data(),
                                                          P, values, &p, dst, g.width));
    size_t bytes = 0;
    Buffer work;
    Status s = hip_status(pcr_hip_rasterize_work_bytes(V, P, g.width, g.height, &bytes));
    if (s.ok()) s = work.allocate(bytes, MemoryLocation::Device);
    if (!s.ok()) return s;
    s = hip_status(pcr_hip_rasterize_polygons(&g, set.coords.data(), V, set.ring_offsets.data(), R, set.polygon_offsets.data(), P, values,
                                              &p, dst, g.width, work.data(), work.bytes(), stream));
    const Status ws = hip_status(pcr_hip_stream_synchronize(stream));             // (the work area is released behind the kernels)
    return s.ok() ? ws : s;
}

PolygonIndex::~PolygonIndex() { reset(); }

void PolygonIndex::reset() {
    if (index_) (void)pcr_hip_polygon_index_destroy(index_);
    index_ = nullptr;
    tables_.release();
}

Status PolygonIndex::build(const PolygonSet& set, const PointInPolygonOptions& options, bool on_device, void* stream) {
    auto refuse = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "points_in_polygons: " + msg); };
    reset();
    const int64_t V = set.num_vertices(), R = set.num_rings(), P = set.num_polygons();
    if (set.coords.size() % 2 != 0) return refuse("coords must hold an x and a y for every vertex");
    if (set.ring_offsets.empty() || set.polygon_offsets.empty()) return refuse("null or inconsistent offsets");
    if (!set.values.empty() && (int64_t)set.values.size() != P) return refuse("values must be empty or one per polygon");
    pcr_hip_polygon_index_params p{};
    p.background = options.background;
    p.index_cols = options.index_cols;
    p.index_rows = options.index_rows;
    p.max_index_bytes = options.max_index_bytes;
    Status s = hip_status(pcr_hip_polygon_index_create(set.coords.data(), V, set.ring_offsets.data(), R, set.polygon_offsets.data(), P,
                                                       set.values.empty() ? nullptr : set.values.data(), &p, &index_));
    if (!s.ok() || !on_device) return s;
    size_t bytes = 0;
    s = hip_status(pcr_hip_polygon_index_info(index_, nullptr, nullptr, nullptr, nullptr, &bytes));
    if (s.ok()) s = tables_.allocate(bytes, MemoryLocation::Device);
    if (s.ok()) s = hip_status(pcr_hip_polygon_index_upload(index_, tables_.data(), tables_.bytes(), stream));
    if (!s.ok()) reset();
    return s;
}

Status PolygonIndex::locate(const double* x, const double* y, size_t n, float* out, bool on_device, void* stream, int threads) const {
    if (!index_) return Status::error(StatusCode::InvalidArgument, "points_in_polygons: no polygons");
    if (on_device) return hip_status(pcr_hip_points_in_polygons(index_, tables_.data(), x, y, n, out, stream, nullptr));
    return hip_status(pcr_hip_points_in_polygons_host(index_, x, y, n, out, threads));
}

namespace {
Status refuse_pipeline(const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: " + msg); }
}  // namespace

Status plan_polygon_channels(const PipelineConfig& cfg) {
    const auto& list = cfg.polygon_channels;
    if (list.empty()) return Status::success();
    if (list.size() > kMaxPolygonChannels)
        return refuse_pipeline("more than " + std::to_string(kMaxPolygonChannels) + " polygon_channels (" + std::to_string(list.size()) + " given)");
    for (size_t i = 0; i < list.size(); ++i) {
        const std::string where = "polygon_channels[" + std::to_string(i) + "]";
        if (list[i].name.empty()) return refuse_pipeline(where + ".name is empty");
        for (size_t k = 0; k < i; ++k)
            if (list[k].name == list[i].name) return refuse_pipeline(where + ".name '" + list[i].name + "' is given twice");
        if (surface_index(cfg, list[i].name) >= 0) return refuse_pipeline(where + ".name '" + list[i].name + "' is also a surface channel");
    }
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0) return refuse_pipeline("polygon_channels are not supported on a row-block shard");
    return Status::success();
}

Status polygon_channels_out_of_core_error() {
    return refuse_pipeline("polygon_channels are not supported on a pipeline that runs out of core");
}

Status store_polygons(const PipelineConfig& cfg, const std::string& name, const PolygonSet& polygons, const PointInPolygonOptions& options,
                      bool on_device, void* stream, PolygonChannels* channels) {
    const int index = polygon_channel_index(cfg, name);
    if (index < 0 || (size_t)index >= channels->size())
        return refuse_pipeline("set_polygons: '" + name + "' names no polygon channel of this pipeline");
    auto made = std::make_unique<PolygonIndex>();
    Status s = made->build(polygons, options, on_device, stream);
    if (s.ok()) (*channels)[(size_t)index] = std::move(made);      // (a refused set leaves the entry as it was)
    return s;
}

Status validate_polygon_channels(const PipelineConfig& cfg, const PointCloud& cloud, const PolygonChannels& channels) {
    for (size_t i = 0; i < cfg.polygon_channels.size(); ++i) {
        const std::string& name = cfg.polygon_channels[i].name;
        if (i >= channels.size() || !channels[i] || !channels[i]->set())
            return refuse_pipeline("polygon channel '" + name + "' has no polygons (call set_polygons first)");
        if (cloud.has_channel(name))
            return refuse_pipeline("the cloud already carries a channel named '" + name + "', which this pipeline derives from polygons");
    }
    return Status::success();
}

}  // namespace detail

Status points_in_polygons(PointCloud& cloud, const PolygonSet& polygons, const std::string& channel, const PointInPolygonOptions& options) {
    auto refuse = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "points_in_polygons: " + msg); };
    if (channel.empty()) return refuse("the output channel needs a name");
    if (const ChannelDesc* d = cloud.channel(channel)) {
        if (d->dtype != DataType::Float32) return refuse("the existing channel '" + channel + "' is not Float32");
    }
    const bool on_device = cloud.location() == MemoryLocation::Device;
    detail::PolygonIndex index;
    Status s = index.build(polygons, options, on_device, nullptr);
    if (!s.ok()) return s;
    if (!cloud.has_channel(channel)) {
        s = cloud.add_channel(channel, DataType::Float32);
        if (!s.ok()) return s;
    }
    const size_t n = cloud.count();
    if (n == 0) return Status::success();
    int threads = 1;
#ifdef _OPENMP
    threads = omp_get_max_threads();
#endif
    s = index.locate(cloud.x(), cloud.y(), n, cloud.channel_f32(channel), on_device, nullptr, threads);
    if (s.ok() && on_device) s = detail::hip_status(pcr_hip_stream_synchronize(nullptr));      // (the tables are released behind the kernel)
    return s;
}

std::unique_ptr<Grid> rasterize_polygons(const PolygonSet& polygons, const GridConfig& grid_config, MemoryLocation location,
                                         const RasterizeOptions& options, Status* status, void* stream) {
    auto fail = [&](const Status& s) {
        if (status) *status = s;
        return std::unique_ptr<Grid>();
    };
    if (grid_config.width <= 0 || grid_config.height <= 0)
        return fail(Status::error(StatusCode::InvalidArgument, "rasterize_polygons: width and height must be positive (compute_dimensions)"));
    if ((int64_t)grid_config.width * grid_config.height > 2147483647LL)
        return fail(Status::error(StatusCode::InvalidArgument, "rasterize_polygons: more than 2^31 - 1 cells"));
    BandDesc d;
    d.name = "label";
    d.dtype = DataType::Float32;
    d.is_state = false;
    std::unique_ptr<Grid> out = Grid::create(grid_config.width, grid_config.height, {d}, location);
    if (!out || !out->band_f32(0)) return fail(Status::error(StatusCode::OutOfMemory, "rasterize_polygons: failed to allocate the grid"));
    (void)out->set_geometry(grid_config);
    const Status s = detail::rasterize_into(polygons, grid_config, options, out->band_f32(0), location, stream);
    if (status) *status = s;
    if (!s.ok()) out.reset();
    return out;
}

}  // namespace pcr
