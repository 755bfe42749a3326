// polygons.h -- (internal) a PolygonSet burnt into a band of memory that already exists: what rasterize_polygons and
// Pipeline::set_zones(name, polygons) share.  The arithmetic is csrc/rasterize.hpp; the contract is in include/pcr_hip.h
// ("polygons").
#pragma once

#include "../../csrc/rasterize.hpp"
#include "buffer.h"
#include "pcr/core/polygons.h"
#include "pcr_hip.h"
#include "sample_grid.h"

#include <memory>
#include <string>
#include <vector>

namespace pcr {
namespace detail {

/// `dst`: geometry.height rows of geometry.width floats, contiguous, in `loc` memory.  Host: the C-ABI's host twin.  Device: the
/// kernels on `stream` with a work area of the call's own, which is released after waiting for the stream.
Status rasterize_into(const PolygonSet& set, const GridConfig& geometry, const RasterizeOptions& options, float* dst,
                      MemoryLocation loc, void* stream);

/// A point-in-polygon index (pcr_hip_polygon_index) and, for a Device user, its tables in HBM: what points_in_polygons builds
/// for one call.  The builder is the C-ABI's (csrc/point_in_polygon_index.hpp); this only holds what it made.
class PolygonIndex {
public:
    PolygonIndex() = default;
    ~PolygonIndex();
    PolygonIndex(const PolygonIndex&) = delete;
    PolygonIndex& operator=(const PolygonIndex&) = delete;
    /// Every refusal, then the index; on_device: the tables uploaded on `stream`, which is waited for once.
    Status build(const PolygonSet& set, const PointInPolygonOptions& options, bool on_device, void* stream);
    /// out[i] for the n points: the kernel on `stream` without a host wait (on_device), or the host twin over `threads` threads.
    Status locate(const double* x, const double* y, size_t n, float* out, bool on_device, void* stream, int threads) const;
    void reset();

    bool set() const { return index_ != nullptr; }

private:
    pcr_hip_polygon_index* index_ = nullptr;
    Buffer tables_;
};

// ---- PipelineConfig::polygon_channels: the checks at create, at set_polygons and at ingest, one message each on every engine
constexpr size_t kMaxPolygonChannels = 8;

/// Index of `name` in cfg.polygon_channels, -1 when it names none (always -1 with the list empty).
inline int polygon_channel_index(const PipelineConfig& cfg, const std::string& name) {
    for (size_t k = 0; k < cfg.polygon_channels.size(); ++k)
        if (cfg.polygon_channels[k].name == name) return (int)k;
    return -1;
}
/// A Float32 channel the pipeline derives itself at ingest: a surface channel or a polygon channel.
inline bool derived_channel(const PipelineConfig& cfg, const std::string& name) {
    return surface_index(cfg, name) >= 0 || polygon_channel_index(cfg, name) >= 0;
}

/// One PolygonIndex per entry of cfg.polygon_channels (empty until set_polygons).
using PolygonChannels = std::vector<std::unique_ptr<PolygonIndex>>;

/// create()'s refusals that do not depend on the engine: an empty or duplicate name, a name that is also a surface channel, more
/// than kMaxPolygonChannels entries, a row-block shard.  An empty list refuses nothing.
Status plan_polygon_channels(const PipelineConfig& cfg);
/// ... and the one of a pipeline that has to run out of core.
Status polygon_channels_out_of_core_error();
/// set_polygons: an unknown name is refused; else the entry's index is built (and uploaded on `stream` for the device).
Status store_polygons(const PipelineConfig& cfg, const std::string& name, const PolygonSet& polygons, const PointInPolygonOptions& options,
                      bool on_device, void* stream, PolygonChannels* channels);
/// ingest's refusals, before any state changes: a polygon channel without polygons, a cloud that already carries the name.
Status validate_polygon_channels(const PipelineConfig& cfg, const PointCloud& cloud, const PolygonChannels& channels);

}  // namespace detail
}  // namespace pcr
