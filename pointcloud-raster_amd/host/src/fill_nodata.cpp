// fill_nodata.cpp -- fill_nodata: the NaN cells of a grid's bands filled where the grid lives (pcr/core/fill_nodata.h).
#include "fill_nodata.h"

#include "buffer.h"
#include "pcr/core/fill_nodata.h"

namespace pcr {

std::unique_ptr<Grid> fill_nodata(const Grid& grid, int radius, const std::vector<int>& bands, Status* status, void* stream) {
    auto fail = [&](StatusCode code, const std::string& msg) {
        if (status) *status = Status::error(code, msg);
        return std::unique_ptr<Grid>();
    };
    if (radius < 1 || radius > detail::fl::kMaxRadius)
        return fail(StatusCode::InvalidArgument, "fill_nodata: radius must be between 1 and 32");
    const int w = grid.cols(), h = grid.rows(), nb = grid.num_bands();
    if (w <= 0 || h <= 0 || nb <= 0) return fail(StatusCode::InvalidArgument, "fill_nodata: empty grid");
    std::vector<char> listed((size_t)nb, bands.empty() ? 1 : 0);
    for (int b : bands) {
        if (b < 0 || b >= nb) return fail(StatusCode::InvalidArgument, "fill_nodata: band index outside the grid");
        listed[(size_t)b] = 1;
    }
    std::vector<BandDesc> descs;
    for (int b = 0; b < nb; ++b) {
        descs.push_back(grid.band_desc(b));
        if (descs.back().dtype != DataType::Float32 || !grid.band_f32(b))
            return fail(StatusCode::InvalidArgument, "fill_nodata needs Float32 bands");
    }
    const MemoryLocation loc = grid.location();
    std::unique_ptr<Grid> out = Grid::create(w, h, descs, loc);
    if (!out) return fail(StatusCode::OutOfMemory, "fill_nodata: failed to allocate the filled grid");
    const bool on_device = loc == MemoryLocation::Device;
    Status s = Status::success();
    for (int b = 0; b < nb && s.ok(); ++b) {
        if (!listed[(size_t)b])
            s = detail::copy_bytes(out->band_f32(b), loc, grid.band_f32(b), loc, (size_t)w * h * sizeof(float), stream);
        else if (on_device)
            s = detail::hip_status(pcr_hip_fill_nodata(grid.band_f32(b), out->band_f32(b), w, h, w, w, radius, stream));
        else
            detail::fill_nodata_host(grid.band_f32(b), out->band_f32(b), w, h, w, w, radius);
    }
    if (s.ok() && on_device) s = detail::hip_status(pcr_hip_stream_synchronize(stream));
    if (status) *status = s;
    if (!s.ok()) out.reset();
    return out;
}

}  // namespace pcr
