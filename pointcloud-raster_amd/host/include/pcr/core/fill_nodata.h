// pcr/core/fill_nodata.h -- no-data (NaN) cells of finished bands filled from their valid neighbours: what gdal_fillnodata is
// run for on a Point-glyph raster, done where the grid lives.  Not in the reference.
//
// The contract, one definition for host and device (csrc/fill_nodata.hpp, include/pcr_hip.h: pcr_hip_fill_nodata): a cell that
// is not NaN is copied bit for bit; a NaN cell becomes the inverse-squared-distance weighted mean of the valid source cells
// within `radius` cells (a disc, 1 <= radius <= 32), summed in binary64 in row-major window order, or stays the NaN it was when
// there is none.  Every read is of the source: filling never chains, a hole wider than 2 * radius keeps a NaN core.
// PipelineConfig::fill_nodata_radius applies it at finalize().
#pragma once

#include "pcr/core/grid.h"
#include "pcr/core/types.h"

#include <memory>
#include <vector>

namespace pcr {

/// A new grid at `grid`'s location with its band descriptions: the bands listed in `bands` (empty: all) filled, the others
/// copied.  Host grids: a loop over rows whose result does not depend on the thread count.  Device grids: pcr_hip_fill_nodata
/// per band on `stream`, synchronised before returning.  nullptr and `status` on failure: InvalidArgument for a radius
/// outside 1..32, a band index outside the grid, or a band that is not Float32.
std::unique_ptr<Grid> fill_nodata(const Grid& grid, int radius, const std::vector<int>& bands = {}, Status* status = nullptr,
                                  void* stream = nullptr);

}  // namespace pcr
