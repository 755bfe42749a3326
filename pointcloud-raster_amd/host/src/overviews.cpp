// overviews.cpp -- build_overviews: the overview levels of a grid, made where the grid lives (pcr/io/grid_io.h).
#include "overviews.h"

#include "buffer.h"
#include "pcr/io/grid_io.h"

namespace pcr {

namespace detail {

Status build_overviews_device(const std::vector<const float*>& d_bands, int width, int height,
                              const std::vector<BandDesc>& descs, int levels, int mode, void* stream,
                              std::vector<std::unique_ptr<Grid>>& out) {
    out.clear();
    for (int k = 1; k <= levels; ++k) {
        auto g = Grid::create(ov::level_extent(width, k), ov::level_extent(height, k), descs, MemoryLocation::Device);
        if (!g) { out.clear(); return Status::error(StatusCode::OutOfMemory, "build_overviews: failed to allocate level " + std::to_string(k)); }
        out.push_back(std::move(g));
    }
    std::vector<float*> dst((size_t)levels);
    for (size_t b = 0; b < d_bands.size(); ++b) {
        for (int k = 0; k < levels; ++k) dst[k] = out[k]->band_f32((int)b);
        Status s = hip_status(pcr_hip_downsample2(d_bands[b], width, height, width, dst.data(), levels, mode, stream));
        if (!s.ok()) { out.clear(); return s; }
    }
    return Status::success();
}

}  // namespace detail

std::vector<std::unique_ptr<Grid>> build_overviews(const Grid& grid, int levels, const std::string& resampling, Status* status,
                                                   void* stream) {
    std::vector<std::unique_ptr<Grid>> out;
    auto done = [&](Status s) {
        if (!s.ok()) out.clear();
        if (status) *status = s;
        return std::move(out);
    };
    if (levels == 0) return done(Status::success());
    const int mode = detail::overview_mode(resampling);
    if (mode < 0) return done(Status::error(StatusCode::InvalidArgument, "unknown overview_resampling: " + resampling));
    const int w = grid.cols(), h = grid.rows(), nb = grid.num_bands();
    if (w <= 0 || h <= 0 || nb <= 0) return done(Status::error(StatusCode::InvalidArgument, "empty grid"));
    const int n = detail::overview_levels(levels, w, h);
    if (n < 0) return done(Status::error(StatusCode::InvalidArgument, "more overview levels than the grid has down to 1x1"));
    if (n == 0) return done(Status::success());
    if (grid.location() != MemoryLocation::Device) return done(detail::build_overviews_host(grid, n, mode, out));
    std::vector<const float*> bands;
    std::vector<BandDesc> descs;
    for (int b = 0; b < nb; ++b) {
        if (!grid.band_f32(b)) return done(Status::error(StatusCode::InvalidArgument, "overviews need Float32 bands"));
        bands.push_back(grid.band_f32(b));
        descs.push_back(grid.band_desc(b));
    }
    Status s = detail::build_overviews_device(bands, w, h, descs, n, mode, stream, out);
    if (s.ok() && !stream) s = detail::hip_status(pcr_hip_stream_synchronize(nullptr));
    return done(s);
}

}  // namespace pcr
