// pcr/core/terrain.h -- what gdaldem derives from a DEM, done where the grid lives: slope, aspect, hillshade, TRI (terrain
// ruggedness index), TPI (topographic position index) and roughness of one band.  Not in the reference.
//
// The contract, one definition for host and device (csrc/terrain.hpp, include/pcr_hip.h: pcr_hip_terrain).  a b c / d e f /
// g h i is the 3 x 3 window around cell e, row a b c being image row r - 1.  NaN is "no data"; every NaN made here is
// 0x7FC00000.  A neighbour outside the image or NaN is missing: by default (gdaldem's) a cell with any missing neighbour is
// NaN, with compute_edges (gdaldem -compute_edges) a missing neighbour takes e's value; e NaN gives NaN in both.
// Gradients are Horn's, in binary64 with the additions in a fixed order and no fused operation:
//   GX = ((c + 2f) + i) - ((a + 2d) + g),  p = GX * z_factor / ( 8 * cell_size_x)
//   GY = ((a + 2b) + c) - ((g + 2h) + i),  q = GY * z_factor / (-8 * cell_size_y),  s2 = p*p + q*q
// with SIGNED cell sizes: on a north-up grid (cell_size_y < 0) p is dz/dEast and q is dz/dNorth.  Each product is rounded to
// Float32 once: SlopeDegrees atan_deg((float)sqrt(s2)); SlopePercent 100 sqrt(s2); Aspect the compass bearing of the downslope
// direction in [0, 360), -1 on flat cells; Hillshade 1 + 254 L clamped below at 1 with
// L = (sin_alt - (p ls + q lc)) / sqrt(1 + s2) (gdaldem's 1..255); TRI the mean absolute difference of the eight neighbours
// from e; TPI e minus the mean of the eight; Roughness max9 - min9.  atan_deg is a binary32 polynomial arctangent written out
// in csrc/terrain.hpp; sqrt and / are correctly rounded.  The result does not depend on threads or tiles: device and host
// agree bit for bit.  PipelineConfig::terrain appends such bands at finalize().
#pragma once

#include "pcr/core/grid.h"
#include "pcr/core/types.h"

#include <memory>
#include <vector>

namespace pcr {

enum class TerrainProduct : uint8_t { SlopeDegrees = 0, SlopePercent = 1, Aspect = 2, Hillshade = 3, TRI = 4, TPI = 5, Roughness = 6 };

/// "slope", "slope_percent", "aspect", "hillshade", "tri", "tpi", "roughness"; "" for a value that is no product.
const char* terrain_product_name(TerrainProduct product);

struct TerrainSpec {
    float z_factor = 1.0f;            // finite, not zero: vertical units per horizontal unit
    bool compute_edges = false;       // a missing neighbour takes the centre's value instead of voiding the cell
    float azimuth = 315.0f;           // hillshade: where the light comes from, degrees clockwise from north; finite
    float altitude = 45.0f;           // hillshade: its height above the horizon, degrees; 0..90
};

/// The hillshade constants every engine and terrain() use, computed once on the host in binary64.
struct TerrainLight {
    double sin_alt, ls, lc;           // sin(altitude), cos(altitude) * sin(azimuth), cos(altitude) * cos(azimuth)
};
TerrainLight terrain_light(double azimuth_deg = 315.0, double altitude_deg = 45.0);

/// A new grid at `grid`'s location with one band per product, in list order, named by terrain_product_name: the products of
/// band `band` of `grid`.  Host grids: an OpenMP loop over rows whose result does not depend on the thread count.  Device
/// grids: pcr_hip_terrain on `stream`, one launch, synchronised before returning.  nullptr and `status` on failure:
/// InvalidArgument for a band index outside the grid, a band that is not Float32, an empty or duplicate product list, a spec
/// outside its ranges or a cell size that is zero or not finite.
std::unique_ptr<Grid> terrain(const Grid& grid, int band, const std::vector<TerrainProduct>& products,
                              const TerrainSpec& spec = TerrainSpec(), double cell_size_x = 1.0, double cell_size_y = -1.0,
                              Status* status = nullptr, void* stream = nullptr);

}  // namespace pcr
