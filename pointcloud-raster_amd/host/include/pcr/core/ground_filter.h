// pcr/core/ground_filter.h -- bare earth from a minimum-elevation band: a progressive morphological filter (Zhang et al. 2003,
// what PDAL's filters.pmf implements) on the grid, done where the grid lives, and height above ground.  Not in the reference.
//
// The contract, one definition for host and device (csrc/ground_filter.hpp, include/pcr_hip.h: pcr_hip_ground_filter).  NaN is
// "no data".  erode(A, R) is the minimum of the non-NaN cells of the (2R + 1)-cell square around a cell, clipped to the image,
// dilate the maximum; NaN cells are ignored, never propagated.  A0 = src; for every level k of the schedule
// Ok = dilate(erode(Ak-1, Rk), Rk), a cell becomes non-ground when Ak-1 - Ok > tk (one binary32 subtraction), Ak = Ok; once
// non-ground, always non-ground.  The DTM keeps the source bits of the cells that stayed ground and is NaN (0x7FC00000)
// everywhere else: where buildings and trees were removed there are holes, which fill_nodata closes.  Minimum and maximum
// are exact, so the result does not depend on threads, tiles or evaluation order: device and host agree bit for bit.
// Height above ground is top - dtm, one binary32 subtraction, NaN (0x7FC00000) where either is.
// PipelineConfig::ground applies both at finalize().
#pragma once

#include "pcr/core/grid.h"
#include "pcr/core/types.h"

#include <memory>
#include <vector>

namespace pcr {

/// The level schedule of the filter; the defaults are PDAL's.
struct GroundFilterSpec {
    int max_radius_cells = 16;        // 1..64: the widest window has 2 * max_radius_cells + 1 cells a side
    bool exponential = true;          // radii 1, 2, 4, ... (false: 1, 2, 3, ...) while <= max_radius_cells
    float slope = 1.0f;               // finite, >= 0
    float initial_distance = 0.15f;   // finite, >= 0: the threshold of the first level
    float max_distance = 2.5f;        // finite, >= initial_distance: no threshold exceeds it
};

/// The schedule both engines and ground_filter() use.  R1 = 1, the next radius 2 R (exponential) or R + 1 while it is
/// <= max_radius_cells;  t1 = (float)min(max_distance, initial_distance),
/// tk = (float)min((double)max_distance, (double)initial_distance + (double)slope * cell_size * 2.0 * (Rk - Rk-1)), evaluated
/// in binary64 in that order and rounded once.  InvalidArgument (naming the field) for a spec outside its ranges or a
/// cell_size that is not finite and positive.
Status ground_filter_levels(const GroundFilterSpec& spec, double cell_size, std::vector<int>* radii, std::vector<float>* thresholds);

/// A new grid at `grid`'s location with the band "dtm": band `band` of `grid` filtered; with top_band >= 0 also the band "hag",
/// top_band - dtm.  Host grids: OpenMP loops whose result does not depend on the thread count.  Device grids:
/// pcr_hip_ground_filter / pcr_hip_band_difference on `stream` with a temporary workspace, synchronised before returning.
/// nullptr and `status` on failure: InvalidArgument for a band index outside the grid, a band that is not Float32, or a spec
/// outside its ranges.
std::unique_ptr<Grid> ground_filter(const Grid& grid, int band, const GroundFilterSpec& spec = GroundFilterSpec(),
                                    double cell_size = 1.0, int top_band = -1, Status* status = nullptr, void* stream = nullptr);

}  // namespace pcr
