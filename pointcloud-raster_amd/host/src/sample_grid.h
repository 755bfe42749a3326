// sample_grid.h -- (internal) what pcr::sample_grid and the pipelines' surface channels share: the checks of
// PipelineConfig::surface_channels at create, of a surface at set_surface and of a cloud at ingest, with one message each on
// every engine, and the host loop of the C-ABI shared out over OpenMP threads.  The arithmetic is csrc/sample_grid.hpp.
#pragma once

#include "buffer.h"
#include "pcr/core/grid.h"
#include "pcr/core/sample_grid.h"
#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"

#include <string>
#include <vector>

namespace pcr {
namespace detail {

constexpr size_t kMaxSurfaceChannels = 8;

/// Index of `name` in cfg.surface_channels, -1 when it names none (always -1 with the list empty).
inline int surface_index(const PipelineConfig& cfg, const std::string& name) {
    for (size_t k = 0; k < cfg.surface_channels.size(); ++k)
        if (cfg.surface_channels[k].name == name) return (int)k;
    return -1;
}

/// The CRS the pipeline's points are in when they are sampled and scattered: the grid's, else target_crs.
inline const CRS& pipeline_crs(const PipelineConfig& cfg) { return cfg.grid.crs.is_valid() ? cfg.grid.crs : cfg.target_crs; }

/// What result() of a whole grid is tagged with (Grid::set_geometry): cfg.grid, its CRS the pipeline's.
inline GridConfig result_geometry(const PipelineConfig& cfg) {
    GridConfig g = cfg.grid;
    g.crs = pipeline_crs(cfg);
    return g;
}

/// create()'s refusals that do not depend on the engine: an empty or duplicate name, a value_channel that is itself a surface
/// channel, an unknown mode, more than kMaxSurfaceChannels entries, a row-block shard.  An empty list refuses nothing.
Status plan_surfaces(const PipelineConfig& cfg);
/// ... and the one of a pipeline that has to run out of core.
Status surfaces_out_of_core_error();

/// One surface of a pipeline: the band in memory the pipeline owns (HBM on the HIP engine, host memory on the host engine)
/// and its geometry as the C-ABI takes it.
struct Surface {
    bool set = false;
    pcr_hip_grid geom{};
    Buffer band;                         // height rows of width floats
};

/// set_surface's refusals -- an unknown name, a grid without geometry, a band outside the grid or not Float32, a CRS identified
/// and not the pipeline's -- and, when it passes, the entry's index and the geometry.
Status check_surface(const PipelineConfig& cfg, const std::string& name, const Grid& grid, int band, int* index, pcr_hip_grid* geom);
/// The checked surface copied into `loc` memory of `out` (on `stream`, which is then waited for when either side is the device).
Status store_surface(const Grid& grid, int band, const pcr_hip_grid& geom, MemoryLocation loc, pcr_hip_stream stream, Surface* out);

/// ingest's refusals, before any state changes: a surface channel with no surface set, a cloud that already carries a channel
/// of that name, a missing or non-Float32 value_channel.
Status validate_surfaces(const PipelineConfig& cfg, const PointCloud& cloud, const std::vector<Surface>& surfaces);

/// The geometry of a grid as the C-ABI takes it (one tile, the whole grid owned).
pcr_hip_grid surface_geom(const GridConfig& g);

/// pcr_hip_sample_grid_host over `threads` OpenMP threads, in chunks (every point is independent: the bits do not depend on
/// how they are shared out).  out may be value.
Status sample_host(const pcr_hip_grid& geom, const float* band, int64_t stride, const double* x, const double* y, const float* value,
                   size_t n, SampleMode mode, float* out, int threads);

}  // namespace detail
}  // namespace pcr
