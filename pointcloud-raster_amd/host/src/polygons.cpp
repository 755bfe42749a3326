// polygons.cpp -- rasterize_polygons: a polygon set burnt into a label grid where the grid is to live (pcr/core/polygons.h).
#include "polygons.h"

#include "pipeline_common.h"

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

}  // namespace detail

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
