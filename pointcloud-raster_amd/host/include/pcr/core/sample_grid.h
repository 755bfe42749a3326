// pcr/core/sample_grid.h -- a band of a grid sampled at the points of a cloud: the way back from a raster to the points
// (extension, no reference counterpart).  The height of every point above a DTM (PDAL's filters.hag_dem, lidR's
// normalize_height) is sample_grid(cloud, dtm, band, "hag", "z").  The contract -- which cell a point reads, how Bilinear
// weighs its neighbours, what is NaN -- is csrc/sample_grid.hpp, the lines the HIP kernel and the host loop both compile.
#pragma once

#include "pcr/core/types.h"

#include <cstdint>
#include <string>

namespace pcr {

class Grid;
class PointCloud;

enum class SampleMode : uint8_t { Nearest, Bilinear };

/// Adds the Float32 channel `out_channel` to the cloud (or overwrites it): the band's sample at every point, or, with a
/// `value_channel`, that channel minus the sample.  out_channel may be value_channel (z -> height above ground, in place).
/// The surface needs a geometry (Grid::set_geometry; a pipeline's result() of a whole grid has one) and may be any grid, not
/// the one the cloud is rasterised into.  Works where the cloud lives -- the kernel for a Device cloud, the host loop (OpenMP,
/// in chunks) otherwise -- and returns when the channel is complete; a band that lives on the other side is copied across
/// first (a band is small, a cloud is not).  The coordinates are sampled as they are: CrsError when the cloud's and the
/// surface's CRS are both identified (crs_epsg) and differ; reproject() the cloud first.  InvalidArgument for a grid without
/// geometry, a band index outside the grid or not Float32, an empty out_channel, a missing or non-Float32 value channel.
Status sample_grid(PointCloud& cloud, const Grid& surface, int band, const std::string& out_channel,
                   const std::string& value_channel = "", SampleMode mode = SampleMode::Bilinear);

}  // namespace pcr
