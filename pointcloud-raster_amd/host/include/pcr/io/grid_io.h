// pcr/io/grid_io.h -- GeoTIFF output of finalized grids (drop-in for the reference's
// include/pcr/io/grid_io.h:15-88: same names, options and argument meaning).
//
// The reference writes through GDAL (src/io/grid_io.cpp), which this image does not have; here the
// files are written directly: little-endian TIFF 6.0 or BigTIFF, IEEE float32 samples, one plane per
// band (PlanarConfiguration = 2, the layout of Grid), strips or tiles, compression NONE / LZW /
// DEFLATE (zlib), GeoTIFF georeferencing (ModelPixelScale + ModelTiepoint, or ModelTransformation
// for south-up grids; GeoKeyDirectory with the EPSG code when the CRS has one) and GDAL's own
// GDAL_METADATA (band descriptions) and GDAL_NODATA ("nan") tags, so that GDAL-based readers see what
// the reference's files show: band names, NaN nodata, geotransform, EPSG.
// Overviews (GeoTiffOptions::overviews): reduced-resolution levels, each a further IFD behind the full image, as GDAL's
// BuildOverviews writes them into the file.  Level k is ceil(w/2) x ceil(h/2) of level k-1 and is made FROM level k-1 (a
// cascade, as GDAL's: level 2 is the average of level-1 averages -- this is the contract, not an approximation); "average"
// is the NaN-aware mean of the 2x2 window, summed ((a + b) + c) + d in binary32 and divided by the number of valid cells,
// "nearest" the window's top-left cell.  build_overviews makes the levels where the grid lives -- for a Device grid in HBM
// (pcr_hip_downsample2), bit for bit what the host loop gives -- and write_geotiff takes them ready-made or builds them.
// Not supported: ZSTD -- NotImplemented.  cloud_optimized -- NotImplemented: the strict COG layout puts the directories
// ahead of the data and this writer appends them; `overviews` gives the same pyramid in an ordinary layout.
#pragma once

#include "pcr/core/grid_config.h"
#include "pcr/core/types.h"

#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace pcr {

class Grid;

struct GeoTiffOptions {
    bool cloud_optimized = false;
    std::string compress = "LZW";          // NONE, LZW, DEFLATE
    int compress_level = 6;                // DEFLATE
    int tile_width = 256;                  // internal TIFF tile (multiple of 16); 0 = strips
    int tile_height = 256;
    bool bigtiff = true;
    std::string overview_resampling = "average";   // "average" or "nearest"; looked at only when overviews != 0
    /// Extension.  0: none.  -1: the reference's rule (levels 2, 4, ... while min(W, H) / level >= 256).  n > 0: exactly
    /// n levels; InvalidArgument when level n-1 is already 1x1.
    int overviews = 0;
};

/// Extension: the overview levels of `grid` (level 1 first), where `grid` lives and with its band descriptions.
/// `levels` as GeoTiffOptions::overviews (0: an empty vector).  Host grids: a loop over output rows whose result does not
/// depend on the thread count.  Device grids: pcr_hip_downsample2 per band on `stream`; synchronised before returning
/// only when `stream` is null.  On failure the vector is empty and *status says why.
std::vector<std::unique_ptr<Grid>> build_overviews(const Grid& grid, int levels, const std::string& resampling,
                                                   Status* status = nullptr, void* stream = nullptr);

/// Grid must be host-resident and match `config` (width x height).  Band names -> band descriptions.
Status write_geotiff(const std::string& path, const Grid& grid, const GridConfig& config,
                     const GeoTiffOptions& options = {});
/// What a pipeline writes to PipelineConfig::output_path with: the defaults, and write_cog = true -> overviews = -1.
inline GeoTiffOptions pipeline_output_options(bool write_cog) {
    GeoTiffOptions o;
    if (write_cog) o.overviews = -1;
    return o;
}
/// The same with the overview levels supplied (host-resident, level 1 first, the cascade's sizes, the grid's band count;
/// otherwise InvalidArgument).  An empty vector with options.overviews != 0: the levels are built here, on the host.
Status write_geotiff(const std::string& path, const Grid& grid, const GridConfig& config, const GeoTiffOptions& options,
                     const std::vector<const Grid*>& overviews);

/// Incremental assembly: reference tiles (GridConfig tiling) in any order; tiles never written
/// read back as nodata.  It never sees the whole image: open() returns nullptr for options.overviews != 0.
class TiledGeoTiffWriter {
public:
    ~TiledGeoTiffWriter();
    static std::unique_ptr<TiledGeoTiffWriter> open(const std::string& path, const GridConfig& config,
                                                    const std::vector<std::string>& band_names,
                                                    const GeoTiffOptions& options = {});
    /// `data`: host, band-sequential [band][row][col] over the tile's own cell range.
    Status write_tile(TileIndex tile, const float* data, int num_bands);
    Status close();

private:
    TiledGeoTiffWriter() = default;
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

/// Reads files written by this writer (and plain float32 strip/tile TIFFs with the same
/// compressions): size, band count, CRS (EPSG only) and bounds from the georeferencing tags.
Status read_geotiff_info(const std::string& path, int& width, int& height, int& num_bands, CRS& crs, BBox& bounds);
Status read_geotiff_band(const std::string& path, int band_index, float* data, int width, int height);
/// Extension: the sizes (width, height) of the overview levels behind the full image, in file order.
Status read_geotiff_overviews(const std::string& path, std::vector<std::pair<int, int>>& sizes);
/// Extension: read_geotiff_band of level `level` (0: the full image).
Status read_geotiff_band_level(const std::string& path, int level, int band_index, float* data, int width, int height);
/// Extension: band descriptions stored by the writer (empty strings when absent).
Status read_geotiff_band_names(const std::string& path, std::vector<std::string>& names);

}  // namespace pcr
