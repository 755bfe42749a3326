// zonal.h -- (internal) what the pipelines share of PipelineConfig::zonal: the checks at create with one message each on every
// engine, the plan (the label band's index, the chosen entries, the column names), the label grids of set_zones, and the one
// routine that makes a table -- through the C-ABI's kernels on device memory, through its host twins on host memory: the folds
// here, the columns from the folded tables in zone_rows.h, which the point zonal tables (point_zonal.h) share.  The arithmetic
// is csrc/zonal.hpp; the contract is in include/pcr_hip.h ("zonal tables").
#pragma once

#include "../../csrc/zonal.hpp"
#include "buffer.h"
#include "cell_stats.h"
#include "ground_filter.h"
#include "histogram.h"
#include "pcr/core/grid.h"
#include "pcr/core/polygons.h"
#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"
#include "terrain.h"
#include "trees.h"

#include <map>
#include <string>
#include <vector>

namespace pcr {
namespace detail {

constexpr size_t kMaxZonal = 4;

/// PipelineConfig::zonal as the engines use it.
struct ZonalPlan {
    struct Entry {
        std::string zones;
        int band = -1;                           // index of the label band in the result grid; -1: an external grid (set_zones)
        std::vector<int> stats, hists;           // indices into the cell-stats and histogram plans
        std::vector<std::vector<float>> q;       // per chosen histogram
        int64_t max_zones = 0;
    };
    std::vector<Entry> entries;
    bool on() const { return !entries.empty(); }
};

/// create()'s refusals (InvalidArgument) and, when it passes, the plan.  An empty list refuses nothing.
Status plan_zonal(const PipelineConfig& cfg, const GroundPlan& ground, const TerrainPlan& terrain, const TreesPlan& trees, ZonalPlan* plan);
/// ... and the one of a pipeline that has to run out of core.
Status zonal_out_of_core_error();

/// The columns of entry i's table in the order of Pipeline.zonal's dict, "zone" and "cells" first.
std::vector<std::string> zonal_column_names(const PipelineConfig& cfg, const ZonalConfig& z);

/// A label grid a set_zones left: rows * width floats in memory the pipeline owns.
struct ZoneGrid {
    Buffer band;
};
/// set_zones' refusals and, when it passes, the copy into `loc` memory (on `stream`, which is then waited for).
Status store_zones(const PipelineConfig& cfg, const std::string& name, const Grid& grid, int band, MemoryLocation loc, void* stream,
                   std::map<std::string, ZoneGrid>* grids);
/// The same with the labels burnt from polygons on cfg.grid, in `loc` memory (polygons.h: rasterize_into): the name's refusal
/// first, then rasterize_polygons' own.
Status store_zones(const PipelineConfig& cfg, const std::string& name, const PolygonSet& polygons, const RasterizeOptions& options,
                   MemoryLocation loc, void* stream, std::map<std::string, ZoneGrid>* grids);

/// What a table is made from: pointers into `device` or host memory, every band and plane rows x width, contiguous.
struct ZonalInputs {
    bool device = false;
    void* stream = nullptr;
    const float* zones = nullptr;
    int width = 0, rows = 0;
    struct Stat {
        const uint32_t* n;
        const long long* s1;
        const unsigned long long* s2;
    };
    std::vector<Stat> stats;                     // by cell-stats entry
    std::vector<const uint32_t*> cubes;          // by histogram
};
/// Entry e's table.  On the device everything is enqueued on in.stream, which is waited for twice: for Z and for the table.
/// with_counts: the histograms' [zone][bin] counts are copied out too.
Status zonal_table(const ZonalPlan::Entry& e, const CellStatsPlan& cstats, const HistogramPlan& hist, const ZonalInputs& in,
                   bool with_counts, ZonalTable* out);

}  // namespace detail
}  // namespace pcr
