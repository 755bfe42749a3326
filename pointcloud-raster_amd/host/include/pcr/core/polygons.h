// pcr/core/polygons.h -- polygons burnt into a label grid, done where the grid is to live: gdal_rasterize's cell-centre rule,
// for the plot and stand maps of the zonal tables (Pipeline::set_zones) and for clipping a cloud to an area (the grid as a
// Nearest surface channel with a filter on it).  Not in the reference.
//
// The contract, one definition for host and device (csrc/rasterize.hpp, include/pcr_hip.h: "polygons").
//   centre   cx(c), cy(r): what GridConfig::cell_to_world returns, bit for bit
//   edge     endpoints ordered so that a.y <= b.y; crosses row r when a.y <= cy(r) < b.y (horizontal edges never do);
//            t = (cy - a.y) / (b.y - a.y), xc = a.x + t * (b.x - a.x), each operation rounded once
//   inside   cell (r, c) is inside a polygon when its crossing edges of row r with xc > cx(c) are odd in number -- all rings of
//            the polygon together (even-odd): holes and multipolygon parts are further rings, orientation plays no part.  A
//            polygon is closed on its low-x and low-y sides and open on the high ones; polygons that share edges (the same
//            vertex bits) and partition a region label each cell centre of it exactly once
//   overlap  the greatest polygon index wins (GDAL's burn order)
//   band     Float32: the winning polygon's value (`values`, or index + 1), `background` elsewhere
//
// points_in_polygons is the same rule with the cell centre replaced by the POINT (csrc/point_in_polygon.hpp, include/pcr_hip.h:
// "polygon index"): the exact clip and the exact tag, where the label grid gives the cell's.  At a cell centre the two agree
// bit for bit.  A NaN coordinate is in no polygon.
// Not done: all_touched, lines and points as geometries, reprojection (run pcr::transform / pcr.transform_xy on the coordinates
// first), shapefile and GeoPackage readers.  (A pipeline derives such a channel at ingest: PipelineConfig::polygon_channels.)
#pragma once

#include "pcr/core/grid.h"
#include "pcr/core/grid_config.h"
#include "pcr/core/point_cloud.h"
#include "pcr/core/types.h"

#include <cstdint>
#include <limits>
#include <memory>
#include <string>
#include <vector>

namespace pcr {

/// P polygons of R rings of V vertices, in the CRS of the grid they are burnt into.
struct PolygonSet {
    std::vector<double> coords;              // x0, y0, x1, y1, ...: 2 * V; rings are closed implicitly
    std::vector<int64_t> ring_offsets;       // R + 1, into the vertices: 0 first, V last, never decreasing
    std::vector<int64_t> polygon_offsets;    // P + 1, into the rings: 0 first, R last, never decreasing
    std::vector<float> values;               // empty: polygon p burns p + 1; else P burn values
    int64_t num_vertices() const { return (int64_t)(coords.size() / 2); }
    int64_t num_rings() const { return ring_offsets.empty() ? 0 : (int64_t)ring_offsets.size() - 1; }
    int64_t num_polygons() const { return polygon_offsets.empty() ? 0 : (int64_t)polygon_offsets.size() - 1; }
};

struct RasterizeOptions {
    float background = std::numeric_limits<float>::quiet_NaN();      // cells outside every polygon
};

/// A one-band Float32 grid "label" of grid_config's width and height at `location`, tagged with the geometry.  Host: the host
/// twin.  Device: the kernels on `stream`, synchronised before the call returns.  nullptr and `status` on failure:
/// InvalidArgument for inconsistent offsets, a ring of fewer than 3 vertices, a coordinate that is not finite or beyond 1e100,
/// values of another length than the polygons, more than 2^31 - 2 polygons or 2^31 - 1 cells, a geometry that is not finite.
std::unique_ptr<Grid> rasterize_polygons(const PolygonSet& polygons, const GridConfig& grid_config,
                                         MemoryLocation location = MemoryLocation::Host,
                                         const RasterizeOptions& options = RasterizeOptions(), Status* status = nullptr,
                                         void* stream = nullptr);

/// The other way round: the zones of band `band` of `grid` as polygons, where the grid lives -- gdal_polygonize's 4-connected
/// outlines: crowns from a tree-id band, a zone map for a GIS.  The contract, one definition for host and device
/// (csrc/polygonize.hpp, include/pcr_hip.h: "polygonize"):
///   zone     the zonal tables' rule: a whole number in [1, 2^24]; NaN, +-Inf, 0, negatives, fractions and greater values are none
///   edge     a side of a zone cell whose neighbour has another zone or none, directed with the cell on its right hand
///   ring     a cycle of the successor rule (right turn first, so a saddle separates: regions are 4-connected), reduced to its
///            corners, from the corner edge of smallest slot 4 * (r * width + c) + side, the ring's key: a simple lattice polygon
///            of at least 4 vertices, no three in a row collinear
///   set      one polygon per zone present, by ascending zone, its rings by ascending key, its value the zone; a polygon is all of
///            its rings under the even-odd rule -- PolygonSet's own meaning: holes and parts are not marked
///   world    corner (i, j) lies at x = min_x + (double)j * cell_size_x, y = max_y + (double)i * cell_size_y of `geometry`
/// so that rasterize_polygons of the result on the same geometry gives the band's zones back cell for cell (where every cell
/// centre rounds strictly between its corners).  Host: the host twin, a sequential trace.  Device: the kernels on `stream`
/// (pointer doubling), which is waited for; only the ring table crosses PCIe.  Both give the same set bit for bit.  A band
/// without a zone gives an empty set.  `geometry` null: the grid's own (Grid::geometry).  An empty set and `status` on failure:
/// InvalidArgument for a band outside the grid or not Float32, no geometry, one whose width and height are not the grid's, more
/// than 2^30 - 1 cells.
/// Not done: 8-connectivity, simplified or smoothed outlines, bands of arbitrary values, shards, out-of-core and sharded
/// pipelines, shapefile or GeoPackage output.
PolygonSet polygonize(const Grid& grid, int band = 0, const GridConfig* geometry = nullptr, Status* status = nullptr,
                      void* stream = nullptr);

struct PointInPolygonOptions {
    float background = std::numeric_limits<float>::quiet_NaN();      // points outside every polygon (any bits are kept)
    int index_cols = 0, index_rows = 0;                              // the index: 0 automatic, or 1 .. 2048 (tests, tuning)
    size_t max_index_bytes = 0;                                      // the cap on the index tables; 0: 256 MiB
};

/// Adds (or overwrites) the Float32 channel `channel` of `cloud`, where the cloud lives: per point the value of the
/// greatest-index polygon that holds it (p + 1, or the set's values), `background` elsewhere.  The polygons are taken to be in
/// the cloud's CRS.  Host: the host twin over the OpenMP thread count.  Device: the index is built on the host, uploaded, and
/// the kernel runs on the default stream, which is waited for.  InvalidArgument for what rasterize_polygons refuses about the
/// set, an empty channel name, an existing channel of another type, an index size outside 0 .. 2048 or over the cap.
Status points_in_polygons(PointCloud& cloud, const PolygonSet& polygons, const std::string& channel = "polygon",
                          const PointInPolygonOptions& options = PointInPolygonOptions());

}  // namespace pcr
