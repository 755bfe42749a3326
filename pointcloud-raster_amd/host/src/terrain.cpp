// terrain.cpp -- terrain_light and terrain: the terrain bands of a band, derived where its grid lives (pcr/core/terrain.h).
#include "terrain.h"

#include "buffer.h"

namespace pcr {

const char* terrain_product_name(TerrainProduct product) {
    static const char* const names[] = {"slope", "slope_percent", "aspect", "hillshade", "tri", "tpi", "roughness"};
    const int k = (int)product;
    return k >= 0 && k < detail::tr::kProducts ? names[k] : "";
}

TerrainLight terrain_light(double azimuth_deg, double altitude_deg) {
    const double rad = 3.14159265358979323846 / 180.0;
    const double cos_alt = std::cos(altitude_deg * rad);
    TerrainLight l;
    l.sin_alt = std::sin(altitude_deg * rad);
    l.ls = cos_alt * std::sin(azimuth_deg * rad);
    l.lc = cos_alt * std::cos(azimuth_deg * rad);
    return l;
}

std::unique_ptr<Grid> terrain(const Grid& grid, int band, const std::vector<TerrainProduct>& products, const TerrainSpec& spec,
                              double cell_size_x, double cell_size_y, Status* status, void* stream) {
    auto fail = [&](const Status& s) {
        if (status) *status = s;
        return std::unique_ptr<Grid>();
    };
    auto refuse = [&](const std::string& msg) { return fail(Status::error(StatusCode::InvalidArgument, msg)); };
    const std::string bad = detail::terrain_spec_error(spec);
    if (!bad.empty()) return refuse("terrain: " + bad);
    if (!detail::terrain_cell_sizes_ok(cell_size_x, cell_size_y)) return refuse("terrain: cell sizes must be finite and not zero");
    if (products.empty()) return refuse("terrain: no product asked for");
    std::vector<int> ids;
    std::vector<BandDesc> descs;
    unsigned mask = 0;
    for (TerrainProduct p : products) {
        const char* name = terrain_product_name(p);
        if (!name[0]) return refuse("terrain: unknown product");
        if (mask & (1u << (int)p)) return refuse(std::string("terrain: duplicate product ") + name);
        mask |= 1u << (int)p;
        ids.push_back((int)p);
        BandDesc d;
        d.name = name;
        d.dtype = DataType::Float32;
        d.is_state = false;
        descs.push_back(d);
    }
    const int w = grid.cols(), h = grid.rows(), nb = grid.num_bands();
    if (w <= 0 || h <= 0 || nb <= 0) return refuse("terrain: empty grid");
    if (band < 0 || band >= nb) return refuse("terrain: band index outside the grid");
    if (grid.band_desc(band).dtype != DataType::Float32 || !grid.band_f32(band)) return refuse("terrain needs a Float32 band");
    const MemoryLocation loc = grid.location();
    std::unique_ptr<Grid> out = Grid::create(w, h, descs, loc);
    if (!out) return fail(Status::error(StatusCode::OutOfMemory, "terrain: failed to allocate the derived grid"));
    std::vector<float*> dsts;
    std::vector<int64_t> strides;
    for (size_t k = 0; k < ids.size(); ++k) {
        dsts.push_back(out->band_f32((int)k));
        strides.push_back(w);
    }
    const int edges = spec.compute_edges ? 1 : 0;
    Status s = Status::success();
    if (loc == MemoryLocation::Device) {
        const TerrainLight l = terrain_light((double)spec.azimuth, (double)spec.altitude);
        s = detail::hip_status(pcr_hip_terrain(grid.band_f32(band), w, h, w, (int)ids.size(), ids.data(), dsts.data(), strides.data(),
                                               cell_size_x, cell_size_y, (double)spec.z_factor, edges, l.sin_alt, l.ls, l.lc, stream));
        const Status ws = detail::hip_status(pcr_hip_stream_synchronize(stream));
        if (s.ok()) s = ws;
    } else {
        detail::terrain_host(grid.band_f32(band), w, h, w, (int)ids.size(), ids.data(), dsts.data(), strides.data(),
                             detail::terrain_consts(spec, cell_size_x, cell_size_y), edges);
    }
    if (status) *status = s;
    if (!s.ok()) out.reset();
    return out;
}

}  // namespace pcr
