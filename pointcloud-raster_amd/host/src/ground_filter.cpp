// ground_filter.cpp -- ground_filter_levels and ground_filter: a band filtered where its grid lives (pcr/core/ground_filter.h).
#include "ground_filter.h"

#include "buffer.h"

namespace pcr {

Status ground_filter_levels(const GroundFilterSpec& spec, double cell_size, std::vector<int>* radii, std::vector<float>* thresholds) {
    if (!radii || !thresholds) return Status::error(StatusCode::InvalidArgument, "ground_filter: null argument");
    const std::string bad = detail::ground_spec_error(spec);
    if (!bad.empty()) return Status::error(StatusCode::InvalidArgument, "ground_filter: " + bad);
    if (!(cell_size > 0.0) || !std::isfinite(cell_size))
        return Status::error(StatusCode::InvalidArgument, "ground_filter: cell_size must be finite and positive");
    detail::ground_levels(spec, cell_size, radii, thresholds);
    return Status::success();
}

std::unique_ptr<Grid> ground_filter(const Grid& grid, int band, const GroundFilterSpec& spec, double cell_size, int top_band,
                                    Status* status, void* stream) {
    auto fail = [&](const Status& s) {
        if (status) *status = s;
        return std::unique_ptr<Grid>();
    };
    auto refuse = [&](const std::string& msg) { return fail(Status::error(StatusCode::InvalidArgument, msg)); };
    std::vector<int> radii;
    std::vector<float> thresholds;
    Status s = ground_filter_levels(spec, cell_size, &radii, &thresholds);
    if (!s.ok()) return fail(s);
    const int w = grid.cols(), h = grid.rows(), nb = grid.num_bands();
    if (w <= 0 || h <= 0 || nb <= 0) return refuse("ground_filter: empty grid");
    if (band < 0 || band >= nb || top_band >= nb) return refuse("ground_filter: band index outside the grid");
    const bool hag = top_band >= 0;
    for (int b : {band, hag ? top_band : band})
        if (grid.band_desc(b).dtype != DataType::Float32 || !grid.band_f32(b)) return refuse("ground_filter needs Float32 bands");
    std::vector<BandDesc> descs(hag ? 2 : 1);
    descs[0].name = "dtm";
    if (hag) descs[1].name = "hag";
    const MemoryLocation loc = grid.location();
    std::unique_ptr<Grid> out = Grid::create(w, h, descs, loc);
    if (!out) return fail(Status::error(StatusCode::OutOfMemory, "ground_filter: failed to allocate the filtered grid"));
    const int levels = (int)radii.size();
    if (loc == MemoryLocation::Device) {
        size_t bytes = 0;
        detail::Buffer work;
        s = detail::hip_status(pcr_hip_ground_filter_work_bytes(w, h, &bytes));
        if (s.ok()) s = work.allocate(bytes, MemoryLocation::Device);
        if (s.ok())
            s = detail::hip_status(pcr_hip_ground_filter(grid.band_f32(band), out->band_f32(0), w, h, w, w, levels, radii.data(),
                                                         thresholds.data(), work.data(), bytes, stream));
        if (s.ok() && hag)
            s = detail::hip_status(pcr_hip_band_difference(grid.band_f32(top_band), out->band_f32(0), out->band_f32(1), w, h, w, w, w,
                                                           stream));
        // (also on failure: the workspace is released below, behind whatever was enqueued)
        const Status ws = detail::hip_status(pcr_hip_stream_synchronize(stream));
        if (s.ok()) s = ws;
    } else {
        detail::ground_filter_host(grid.band_f32(band), out->band_f32(0), w, h, w, w, levels, radii.data(), thresholds.data());
        if (hag) detail::band_difference_host(grid.band_f32(top_band), out->band_f32(0), out->band_f32(1), w, h, w, w, w);
    }
    if (status) *status = s;
    if (!s.ok()) out.reset();
    return out;
}

}  // namespace pcr
