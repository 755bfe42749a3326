// host_pipeline.h -- (internal) Pipeline::Host: the pipeline on the host engine (host_engine.h), behind ExecutionMode::CPU,
// Auto without a GPU and gpu_fallback_to_cpu -- what the reference does in those cases (src/engine/pipeline.cpp:100-131).
// Same validation, messages, band naming, progress callback and `.pcrt` checkpoints as the HIP pipeline.
#pragma once

#include "cell_stats.h"
#include "extremes.h"
#include "histogram.h"
#include "host_engine.h"
#include "pcr/core/grid.h"
#include "pcr/engine/pipeline.h"
#include "pipeline_common.h"
#include "point_zonal.h"
#include "polygons.h"
#include "sample_grid.h"
#include "zonal.h"

#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace pcr {

struct Pipeline::Host {
    struct Group : detail::GroupSpec {   // one pass over the points (detail::plan_groups) and its planes
        detail::HostPlanes planes;
    };
    using Output = detail::Output;

    PipelineConfig cfg;
    std::unique_ptr<detail::HostEngine> engine;
    std::vector<Group> groups;
    std::vector<Output> outputs;
    detail::FilterPlan filters;          // ReductionSpec::filter of every spec, planned at init
    std::vector<detail::Surface> surfaces;   // PipelineConfig::surface_channels, entry by entry: the band in host memory
    detail::PolygonChannels polygon_sets;    // PipelineConfig::polygon_channels, entry by entry: the index (set_polygons)
    detail::HistogramPlan hist;          // PipelineConfig::histograms, planned at init
    std::vector<std::vector<uint32_t>> cubes;    // entry by entry: count[bins][height * width], zero at create
    detail::ExtremesPlan ext;            // PipelineConfig::extremes, planned at init
    std::vector<std::vector<uint32_t>> ext_keys; // entry by entry: keys[k][height * width], all EMPTY (0xFFFFFFFF) at create
    detail::CellStatsPlan cstats;         // PipelineConfig::cell_stats, planned at init
    struct StatPlanes {                  // entry by entry: N, S1, S2 over height * width, zero at create
        std::vector<uint32_t> n;
        std::vector<int64_t> s1;
        std::vector<uint64_t> s2;
    };
    std::vector<StatPlanes> stat_planes;
    std::unique_ptr<Grid> result;
    bool finalized = false;
    std::vector<TreeTable> tree_tables;      // PipelineConfig::trees, entry by entry, as the last finalize left them
    std::vector<Status> tree_status;
    detail::ZonalPlan zonal_plan;            // PipelineConfig::zonal, planned at init
    std::map<std::string, detail::ZoneGrid> zone_grids;   // the label grids of set_zones, by name, in host memory
    bool zonal_fresh = false;                // the last finalize's bands and the planes belong together: no ingest since
    detail::PointZonalPlan pz_plan;          // PipelineConfig::point_zonal, planned at init
    detail::PointZonalState pz_state;        // its tables in host memory, zero at create, added to by every ingest
    ProgressCallback callback;
    size_t collections = 0, points = 0;
    ScatterInfo last{};
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();

    Status init();
    Status ingest(const PointCloud& cloud);
    Status finalize();
    Status set_surface(const std::string& name, const Grid& grid, int band);
    Status set_polygons(const std::string& name, const PolygonSet& polygons, const PointInPolygonOptions& options);
    Status set_zones(const std::string& name, const Grid& grid, int band);
    Status set_zones(const std::string& name, const PolygonSet& polygons, const RasterizeOptions& options);
    Status zonal(int i, ZonalTable* out, bool with_counts) const;
    Status polygonize(const std::string& band_name, PolygonSet* out) const;
    Status point_zonal(int i, PointZonalTable* out, bool with_counts) const;
    Status save_state(const std::string& dir);
    Status load_state(const std::string& dir);
    ProgressInfo stats() const;
};

}  // namespace pcr
