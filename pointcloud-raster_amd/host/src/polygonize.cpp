// polygonize.cpp -- polygonize: the zones of a label band as a polygon set, made where the band lives (pcr/core/polygons.h).
#include "polygonize.h"

#include "pipeline_common.h"
#include "zone_rows.h"

#include <algorithm>
#include <numeric>

namespace pcr {
namespace detail {

namespace {

namespace pg = pcrhip::polygonize;

// The ring table on the host, from the kernels: E, then R and V, are the only values waited for.
Status rings_device(const float* band, int W, int H, void* stream, pg::HostRings* t) {
    size_t bytes = 0;
    Status s = hip_status(pcr_hip_polygonize_cells_work_bytes(W, H, &bytes));
    Buffer cells, rings;
    if (s.ok()) s = cells.allocate(bytes, MemoryLocation::Device);
    if (!s.ok()) return s;
    int64_t E = 0, R = 0, V = 0;
    s = hip_status(pcr_hip_polygonize_edges(band, W, H, W, cells.data(), cells.bytes(), stream));
    const Status cs = hip_status(pcr_hip_polygonize_count(cells.data(), cells.bytes(), &E, nullptr, nullptr, nullptr, nullptr, stream));
    if (!s.ok() || !cs.ok()) return s.ok() ? cs : s;
    t->edges = E;
    if (E == 0) return Status::success();
    s = hip_status(pcr_hip_polygonize_rings_work_bytes(E, &bytes));
    if (s.ok()) s = rings.allocate(bytes, MemoryLocation::Device);
    if (!s.ok()) return s;
    s = hip_status(pcr_hip_polygonize_rings(band, W, H, W, cells.data(), cells.bytes(), E, rings.data(), rings.bytes(), nullptr, stream));
    Status ws = hip_status(pcr_hip_polygonize_count(cells.data(), cells.bytes(), &E, &R, &V, nullptr, nullptr, stream));
    if (!s.ok() || !ws.ok()) return s.ok() ? ws : s;
    if (R < 1 || V < 4 * R || V > E) return Status::error(StatusCode::CudaError, "polygonize: inconsistent ring counts");

    Arena a;                                                         // the table in HBM: zone, offset, row, col
    const size_t table = Arena::padded((size_t)R * 4) + Arena::padded(((size_t)R + 1) * 8) + 2 * Arena::padded((size_t)V * 4);
    if (!(s = a.buf.allocate(table, MemoryLocation::Device)).ok()) return s;
    int64_t* d_offset = a.take<int64_t>((size_t)R + 1);
    uint32_t* d_zone = a.take<uint32_t>((size_t)R);
    int32_t* d_row = a.take<int32_t>((size_t)V);
    int32_t* d_col = a.take<int32_t>((size_t)V);
    s = hip_status(pcr_hip_polygonize_fetch(band, W, H, W, cells.data(), cells.bytes(), E, rings.data(), rings.bytes(), R, V, d_zone,
                                            d_offset, d_row, d_col, stream));
    t->ring_zone.resize((size_t)R);
    t->ring_offset.resize((size_t)R + 1);
    t->vertex_row.resize((size_t)V);
    t->vertex_col.resize((size_t)V);
    const MemoryLocation host = MemoryLocation::Host, dev = MemoryLocation::Device;
    if (s.ok()) s = copy_bytes(t->ring_zone.data(), host, d_zone, dev, (size_t)R * 4, stream);
    if (s.ok()) s = copy_bytes(t->ring_offset.data(), host, d_offset, dev, ((size_t)R + 1) * 8, stream);
    if (s.ok()) s = copy_bytes(t->vertex_row.data(), host, d_row, dev, (size_t)V * 4, stream);
    if (s.ok()) s = copy_bytes(t->vertex_col.data(), host, d_col, dev, (size_t)V * 4, stream);
    ws = hip_status(pcr_hip_stream_synchronize(stream));             // (the work areas are released behind what was enqueued)
    return s.ok() ? ws : s;
}

}  // namespace

Status polygonize_band(const float* band, const GridConfig& geometry, MemoryLocation loc, void* stream, PolygonSet* out) {
    *out = PolygonSet();
    out->ring_offsets.assign(1, 0);
    out->polygon_offsets.assign(1, 0);
    const int W = geometry.width, H = geometry.height;
    size_t bytes = 0;                                                // (the extent's refusals, in the C-ABI's words)
    Status s = hip_status(pcr_hip_polygonize_cells_work_bytes(W, H, &bytes));
    if (!s.ok()) return s;
    pg::HostRings t;
    if (loc == MemoryLocation::Device) s = rings_device(band, W, H, stream, &t);
    else pg::host(pg::Band{band, W, H, W}, &t);
    if (!s.ok()) return s;

    // the one pass: rings by zone, stable, so that a polygon's rings stay in key order
    const size_t R = t.ring_zone.size();
    std::vector<uint32_t> order(R);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return t.ring_zone[x] < t.ring_zone[y]; });
    const double min_x = geometry.bounds.min_x, max_y = geometry.bounds.max_y;
    out->coords.reserve(2 * t.vertex_row.size());
    for (size_t k = 0; k < R; ++k) {
        const uint32_t j = order[k];
        if (k > 0 && t.ring_zone[j] != t.ring_zone[order[k - 1]]) out->polygon_offsets.push_back((int64_t)k);
        if (k == 0 || t.ring_zone[j] != t.ring_zone[order[k - 1]]) out->values.push_back((float)t.ring_zone[j]);
        for (int64_t v = t.ring_offset[j]; v < t.ring_offset[j + 1]; ++v) {
            out->coords.push_back(pg::world_x(min_x, geometry.cell_size_x, t.vertex_col[(size_t)v]));
            out->coords.push_back(pg::world_y(max_y, geometry.cell_size_y, t.vertex_row[(size_t)v]));
        }
        out->ring_offsets.push_back((int64_t)(out->coords.size() / 2));
    }
    if (R > 0) out->polygon_offsets.push_back((int64_t)R);
    return Status::success();
}

Status polygonize_check(const PipelineConfig& cfg, const PolygonSet* out, bool fresh, const Grid* result, const std::string& band_name,
                        int* band) {
    auto refuse = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: polygonize: " + msg); };
    if (!out) return refuse("null argument");
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0) return refuse("not on a row-block shard");
    if (!fresh || !result) return refuse("no band '" + band_name + "' (of a finalize with no ingest since)");
    *band = result->band_index(band_name);
    if (*band < 0 || !result->band_f32(*band)) return refuse("'" + band_name + "' names no Float32 band of the result");
    if (result->cols() != cfg.grid.width || result->rows() != cfg.grid.height) return refuse("the result is not the whole grid");
    return Status::success();
}

}  // namespace detail

PolygonSet polygonize(const Grid& grid, int band, const GridConfig* geometry, Status* status, void* stream) {
    PolygonSet out;
    out.ring_offsets.assign(1, 0);
    out.polygon_offsets.assign(1, 0);
    auto done = [&](const Status& s) {
        if (status) *status = s;
        return out;
    };
    auto refuse = [&](const std::string& msg) { return done(Status::error(StatusCode::InvalidArgument, "polygonize: " + msg)); };
    if (band < 0 || band >= grid.num_bands()) return refuse("band index outside the grid");
    if (grid.band_desc(band).dtype != DataType::Float32 || !grid.band_f32(band)) return refuse("the band must be Float32");
    if (!geometry) geometry = grid.geometry();
    if (!geometry) return refuse("the grid has no geometry (Grid::set_geometry) and none was given");
    if (geometry->width != grid.cols() || geometry->height != grid.rows()) return refuse("the geometry's width and height are not the grid's");
    return done(detail::polygonize_band(grid.band_f32(band), *geometry, grid.location(), stream, &out));
}

}  // namespace pcr
