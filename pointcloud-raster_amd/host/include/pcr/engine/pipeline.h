// pcr/engine/pipeline.h -- the public engine API (drop-in for the reference's
// include/pcr/engine/pipeline.h:20-145): ReductionSpec, ExecutionMode, PipelineConfig,
// ProgressInfo, Pipeline{create, validate, ingest, finalize, run, set_progress_callback,
// result, stats}.  Behind it: the MI355X HIP engine (include/pcr_hip.h) for GPU / Auto / Hybrid,
// and a host engine for ExecutionMode::CPU and for the cases in which the reference falls back to
// its CPU mode (no device + gpu_fallback_to_cpu, Auto without a GPU: src/engine/pipeline.cpp:100-131)
// -- announced on stderr with the reference's own Warning / Info line, visible through engine(),
// and forbidden altogether by PCR_REQUIRE_GPU_ENGINE=1.
#pragma once

#include "pcr/core/grid_config.h"
#include "pcr/core/ground_filter.h"
#include "pcr/core/polygons.h"
#include "pcr/core/sample_grid.h"
#include "pcr/core/terrain.h"
#include "pcr/core/trees.h"
#include "pcr/core/types.h"
#include "pcr/engine/filter.h"
#include "pcr/engine/glyph.h"

#include <functional>
#include <memory>
#include <string>
#include <vector>

namespace pcr {

class PointCloud;
class Grid;
struct LasOptions;

struct ReductionSpec {
    std::string value_channel;
    ReductionType type = ReductionType::Sum;
    std::string weight_channel;        // declared; WeightedAverage uses weight 1 with the Point glyph (reference behaviour)
    // MostRecent (Point glyph only): the Float32 channel whose greatest value picks the cell's point -- "newest survey wins".
    // Points with a NaN or <= -FLT_MAX timestamp are ignored; among equal timestamps the greater value wins, so the result
    // does not depend on the order, the engine or the split of the points.  Required for MostRecent, unused otherwise.
    std::string timestamp_channel;
    float percentile = 0.5f;
    std::string output_band_name;      // default "{value_channel}_{int(type)}"
    GlyphSpec glyph;
    // Extension (not in the reference; empty = reference behaviour): this reduction folds only the points that pass
    // PipelineConfig::filter AND this filter -- a DTM (Min of z over class 2), a DSM (Max of z over first returns) and an
    // intensity average over single returns come out of ONE ingest.  Any glyph.  Specs group into one pass only when their
    // filters are equal too (the same predicates in the same order).  The pipeline keeps ONE set of touched-tile flags, set by
    // PipelineConfig::filter's survivors alone: this filter never sets or clears a flag, so a filtered Sum is 0 -- not NaN,
    // as a pipeline of its own would say -- in a tile that only other points touched (Count, Average, Max, Min and MostRecent
    // are NaN in empty cells either way), and the shards' flag all-reduce, the `.pcrt` "touched tile" rule and merge_touched
    // stay as they are.  stats().points_processed counts PipelineConfig::filter's survivors; checkpoints record no filter.
    // create() refuses more than 8 distinct non-empty filters, a conjunction (pipeline filter + this one) of more than 16
    // predicates and more than 32 distinct predicates in all; ingest() checks the channels like PipelineConfig::filter's.
    FilterSpec filter;
};

enum class ExecutionMode : uint8_t { CPU, GPU, Auto, Hybrid };

/// PipelineConfig::ground: the ground filter (pcr/core/ground_filter.h) at finalize().  Bands are named as the result grid
/// names them (ReductionSpec::output_band_name, or "{value_channel}_{int(type)}").
struct GroundFilterConfig : GroundFilterSpec {
    std::string source_band;             // the band filtered, normally a Min band; empty: off
    std::string top_band;                // hag = this band - DTM, normally a Max band; empty: no hag band
    std::string dtm_band_name = "dtm";   // the name of the appended DTM band
    std::string hag_band_name = "hag";   // the name of the appended hag band
};

/// One entry of PipelineConfig::terrain: one terrain band (pcr/core/terrain.h) appended at finalize().
struct TerrainBandConfig : TerrainSpec {
    std::string source_band;             // any band of the result by name, the ground filter's DTM and hag bands included
    TerrainProduct product = TerrainProduct::Hillshade;
    std::string band_name;               // default "{source_band}_{terrain_product_name(product)}"
};

/// One entry of PipelineConfig::trees: the tree_id and tree_height bands (pcr/core/trees.h) of one band, appended at finalize().
struct TreeBandConfig : TreeSpec {
    std::string source_band;             // a reduction, percentile, extremes or cell-stats band, the DTM or the hag band, by name
    std::string id_band_name;            // default "{source_band}_tree_id"
    std::string height_band_name;        // default "{source_band}_tree_height"
};

/// One entry of PipelineConfig::polygon_channels: a per-point Float32 channel the pipeline derives at ingest from the polygons
/// given with Pipeline::set_polygons -- the value of the greatest-index polygon that holds the point, exactly
/// (pcr/core/polygons.h: points_in_polygons).
struct PolygonChannelConfig {
    std::string name;                    // the channel: usable wherever a Float32 channel is named
};

/// One entry of PipelineConfig::surface_channels: a per-point Float32 channel the pipeline derives at ingest from a finished
/// band (Pipeline::set_surface) -- the band's sample at the point, or, with a value_channel, that channel minus the sample
/// (z and a DTM: the height above ground).  The contract is pcr/core/sample_grid.h's.
struct SurfaceChannelConfig {
    std::string name;                    // the channel's name: whatever names a Float32 channel may name it
    std::string value_channel;           // a Float32 channel of the cloud; empty: the sample itself
    SampleMode mode = SampleMode::Bilinear;
};

/// One entry of PipelineConfig::histograms: a per-cell histogram of one channel, accumulated at ingest beside the reductions,
/// and the percentile bands finalize() walks out of it.  The contract (include/pcr_hip.h, "per-cell histograms"):
///   accepted   a point is accepted when it is routed to a cell by the rule of the Point glyph (inclusive bounds, true-division
///              routing, after reprojection and surface channels), is kept by PipelineConfig::filter AND by `filter`, and its
///              value is not NaN.
///   bin        binary64: inv_w = (double)bins / ((double)hi - (double)lo) is computed once; t = ((double)v - (double)lo) * inv_w;
///              b = 0 if t < 0, bins - 1 if t >= bins, else (int)t.  Out-of-range values and +-Inf are clamped into the end
///              bins: counted, not dropped.
///   state      each accepted point adds 1 to count[b][cell], uint32: a cube of bin planes in the state window's layout, zero
///              at create.  A counter wraps at 2^32 (documented, not checked).
///   band for q per cell, with N = sum of count[b]: NaN where N == 0 (touched-tile flags play no part); else
///              k = min(max((int64)ceil((double)q * (double)N), 1), N), b the smallest bin with cumulative count C_b >= k, and
///              band = (float)((double)lo + w * ((double)b + ((double)(k - C_{b-1}) - 0.5) / (double)count[b])) with
///              w = ((double)hi - (double)lo) / bins computed once, every operation rounded on its own.  A single point in a
///              bin gives the bin's centre; the band is monotone in q.
/// Both engines and both device paths give the same bits for any order, chunking or number of ingests.
struct HistogramConfig {
    std::string value_channel;           // any Float32 channel, a surface channel ("hag") included
    float lo = 0.f, hi = 64.f;           // bin b covers [lo + b*w, lo + (b+1)*w), w = (hi-lo)/bins
    int bins = 32;                       // 1..256
    FilterSpec filter;                   // like ReductionSpec::filter: AND PipelineConfig::filter
    std::vector<float> percentiles;      // each in [0,1]; one band per entry, in order; may be empty
    std::vector<std::string> band_names; // default "{value_channel}_p{round(q*100)}", e.g. "hag_p95"
};

/// Which end of a cell's values an ExtremesConfig keeps.
enum class ExtremeSide : int { Lowest = 0, Highest = 1 };

/// One entry of PipelineConfig::extremes: the k lowest (or highest) DISTINCT values of one channel per cell, kept at ingest
/// beside the reductions, and the outlier-free Min (Max) band finalize() walks out of them -- what PDAL's filters.elm
/// (extended local minimum) does ahead of a ground filter, as a band.  The contract (include/pcr_hip.h, "per-cell extremes"):
///   accepted   exactly the histograms' rule: routed to a cell by the rule of the Point glyph (after reprojection and surface
///              channels), kept by PipelineConfig::filter AND by `filter`, value not NaN.  +-Inf are values.
///   key        the bits of v, -0.0 folded to +0.0 on the bits, then ord() (the MostRecent fold's order-preserving map) for
///              Lowest, ~ord() for Highest.  Every real value's key lies in [0x007FFFFF, 0xFF800000]; EMPTY = 0xFFFFFFFF.
///   state      k planes of uint32 keys in the state window's layout, all EMPTY at create; plane j of a cell holds the (j+1)-th
///              smallest distinct key among the cell's accepted points, or EMPTY.  Distinct values, not points: the state is
///              a set, hence order-independent, and two noise returns at one height count as one level.
///   band       with n filled slots and v[i] the decoded floats: NaN where n == 0 (touched-tile flags play no part); else
///              start at i = 0 and advance while i + 1 < n and d > max_gap, d being one binary32 subtraction (v[i+1] - v[i]
///              for Lowest, v[i] - v[i+1] for Highest); the band is v[i].  max_gap = +Inf gives the plain Min or Max.  A cell
///              whose k kept values are ALL more than max_gap apart yields the k-th: with k - 1 or more isolated outliers in
///              one cell the band is the last value kept, whatever it is -- raise k where that can happen.
/// Both engines and both device paths give the same bits for any order, chunking or number of ingests.
struct ExtremesConfig {
    std::string value_channel;           // any Float32 channel, a surface channel ("hag") included
    ExtremeSide side = ExtremeSide::Lowest;
    int k = 4;                           // 2..8 values kept per cell
    float max_gap = 1.0f;                // >= 0; +Inf: the plain Min / Max
    FilterSpec filter;                   // like ReductionSpec::filter: AND PipelineConfig::filter
    std::string band_name;               // default "{value_channel}_low" / "{value_channel}_high"
};

/// A band a CellStatsConfig makes.
enum class CellStat : int { Mean = 0, Variance = 1, StdDev = 2 };

/// One entry of PipelineConfig::cell_stats: the exact mean, variance and standard deviation of one channel per cell -- surface
/// roughness, canopy structure (lidR's zsd), the vertical noise a survey's QA asks for.  A float32 Sum(v^2)/N - mean^2 is wrong
/// by metres for z ~ 1500 m, sigma ~ 0.1 m; lidar values are fixed-point at the source, so the value is quantized to an integer
/// step and N, the sum and the sum of squares are kept in integers.  The contract (include/pcr_hip.h, "per-cell stats"):
///   accepted   exactly the histograms' rule: routed to a cell by the rule of the Point glyph (after reprojection and surface
///              channels), kept by PipelineConfig::filter AND by `filter`, value not NaN.
///   step       t = ((double)v - origin) * (1.0 / resolution); with Q = 2^21: q = -Q if t <= -Q, Q if t >= Q, else rint(t), ties
///              to even.  Values out of range and +-Inf are clamped and counted.  At the default 1 cm step: +-20.9 km.
///   state      three planes in the state window's layout, zero at create: N (uint32), S1 = sum q (int64), S2 = sum q^2
///              (uint64).  S2 is exact for at least 2^22 accepted points per cell, N wraps at 2^32: documented, not checked.
///   bands      NaN where N == 0.  Mean = (float)(origin + resolution * ((double)S1 / (double)N)).  Variance and StdDev: NaN where
///              N <= ddof; else D = N * S2 - S1^2, an exact 128-bit integer, vq = (double)D / ((double)N * (double)(N - ddof)),
///              Variance = (float)(resolution^2 * vq), StdDev = (float)(resolution * sqrt(vq)).
/// Both engines and both device paths give the same bits for any order, chunking or number of ingests.
struct CellStatsConfig {
    std::string value_channel;           // any Float32 channel, a surface channel ("hag") included
    double origin = 0.0;                 // finite; the value whose step is 0
    double resolution = 0.01;            // finite, > 0: the step
    std::vector<CellStat> products{CellStat::StdDev};    // 1..3, no duplicate: one band each, in this order
    int ddof = 0;                        // 0 population, 1 sample
    FilterSpec filter;                   // like ReductionSpec::filter: AND PipelineConfig::filter
    std::vector<std::string> band_names; // default "{value_channel}_mean" / "_var" / "_std"
};

/// One entry of PipelineConfig::zonal: a table with one row per zone -- per tree with a tree_id band, per plot or stand with a
/// rasterized label grid -- of the chosen cell-stats entries and histograms, folded where their state lives (lidR's
/// crown_metrics and plot_metrics).  The contract (include/pcr_hip.h, "zonal tables"; csrc/zonal.hpp):
///   zone       of a cell: the label when it is a whole number in [1, 2^24], else none (NaN, +-Inf, 0, negatives, 2.5).  Z is the
///              greatest zone present; row k of the table is zone k + 1; a zone no cell carries has cells = 0.
///   fold       64-bit integer sums of the cells' N, S1, S2 and of their histogram counts, modulo 2^64.
///   rows       mean, var, std: the cell-stats bands' arithmetic on the zone's sums, with the entry's origin, resolution and
///              ddof; percentiles: the percentile bands' walk over the zone's counts.  NaN where the zone has no point.
/// Both engines give the same bits.
struct ZonalConfig {
    std::string zones;                   // a band of the result by name (normally "{source}_tree_id"), or, with `external`, the
                                         // name of a label grid given by Pipeline::set_zones
    bool external = false;
    std::vector<int> cell_stats;         // indices into PipelineConfig::cell_stats
    std::vector<int> histograms;         // indices into PipelineConfig::histograms
    bool own_percentiles = true;         // every chosen histogram with its entry's own percentile list; false: `percentiles`
    std::vector<float> percentiles;      // each in [0, 1], at most 16
    int max_zones = 1 << 22;             // 1..2^24: Pipeline::zonal answers OutOfRange for a band with a greater zone
};

/// Pipeline::zonal's table: rows 0 .. size() - 1 are zones 1 .. size().
struct ZonalTable {
    struct StatColumns {                 // one per chosen cell-stats entry: "{channel}_n", "_mean", "_var", "_std"
        std::string channel;
        std::vector<uint64_t> n;
        std::vector<float> mean, var, stddev;
    };
    struct HistColumns {                 // one per chosen histogram: "{channel}_hist_n", "{channel}_p{round(q * 100)}"
        std::string channel;
        int bins = 0;
        std::vector<uint64_t> hist_n;
        std::vector<float> q;
        std::vector<std::vector<float>> p;       // p[j]: the column of q[j]
        std::vector<uint64_t> counts;            // [zone][bin]; filled only when asked for (Pipeline::zonal, with_counts)
    };
    std::vector<int32_t> zone;
    std::vector<int64_t> cells;
    std::vector<StatColumns> stats;
    std::vector<HistColumns> hists;
    size_t size() const { return zone.size(); }
};

/// One entry of PipelineConfig::point_zonal: a table with one row per zone of a per-point LABEL CHANNEL -- the returns of each plot
/// (a polygon channel: exactly those inside it), of each tree (a Nearest surface channel over a tree_id band), of each flight line
/// (`point_source_id`) or class (`classification`) -- folded at every ingest: lidR's plot_metrics and crown_metrics as a group-by
/// over POINTS, where PipelineConfig::zonal gives a return the zone of its cell.  The contract (include/pcr_hip.h, "point zonal
/// tables"; csrc/point_zonal.hpp):
///   zone       of a point: the label when it is a whole number in [1, 2^24], else none (NaN, +-Inf, 0, negatives, 2.5).  The
///              table has max_zones rows of state; a kept point with a greater zone is counted as overflow and makes
///              Pipeline::point_zonal answer OutOfRange.
///   accepted   a point that PipelineConfig::filter AND the spec's filter keep, whose zone is in 1..max_zones and whose value is
///              not NaN.  THE GRID PLAYS NO PART: x and y are not read, a point outside the grid but inside a plot counts.
///   fold       64-bit integers modulo 2^64, accumulated over every ingest: points per zone (PipelineConfig::filter's survivors,
///              whatever their value), per stats spec n, the sum of the steps and of their squares (CellStatsConfig's step), per
///              histogram the counts of HistogramConfig's bins.
///   rows       ZonalConfig's: the same columns from the same arithmetic, up to the greatest zone a point carried.
/// The specs are OWNED: their value_channel, origin, resolution and ddof, or lo, hi, bins and percentiles, and their filter mean
/// what they mean per cell, but no per-cell plane is allocated for them and products and band_names are not read.  Both engines
/// give the same bits for any order, chunking or number of ingests.
struct PointZonalConfig {
    std::string label_channel;           // any Float32 channel: a polygon channel, a surface channel, or the cloud's own
    std::vector<CellStatsConfig> cell_stats;     // at most 4
    std::vector<HistogramConfig> histograms;     // at most 4
    int max_zones = 1 << 16;             // 1..2^24: the rows of state kept
};

/// Pipeline::point_zonal's table: rows 0 .. size() - 1 are zones 1 .. size(), the columns ZonalTable's with `points` for `cells`.
struct PointZonalTable {
    std::vector<int32_t> zone;
    std::vector<int64_t> points;
    std::vector<ZonalTable::StatColumns> stats;
    std::vector<ZonalTable::HistColumns> hists;
    size_t size() const { return zone.size(); }
};

struct PipelineConfig {
    GridConfig grid;
    std::vector<ReductionSpec> reductions;
    FilterSpec filter;

    CRS target_crs;
    bool auto_reproject = true;

    ExecutionMode exec_mode = ExecutionMode::Auto;   // GPU, Auto and Hybrid run the HIP engine; CPU the host engine

    // A grid whose accumulation state (4 B per cell and plane, + the finalized bands) exceeds gpu_memory_budget (0 = ~80 %
    // of the free GPU memory) is processed OUT OF CORE: in row bands of whole reference-tile rows, one band's state in HBM at
    // a time, the others in host memory up to host_cache_budget (0 = ~50 % of the free host memory), beyond that in files
    // under state_dir (a temporary directory when empty) -- the role of the reference's TileManager LRU + disk spill
    // (src/engine/tile_manager.cpp:76-375).
    size_t gpu_memory_budget = 0;
    size_t host_cache_budget = 0;
    size_t chunk_size = 0;

    size_t gpu_pool_size_bytes = 512 * 1024 * 1024;  // initial scratch arena of the engine
    int cuda_device_id = 0;                          // HIP device ordinal
    bool use_cuda_streams = true;
    bool gpu_fallback_to_cpu = true;                 // GPU mode without a usable device continues on the host engine (with a Warning)
    bool gpu_require_strict = false;

    size_t cpu_threads = 0;                          // host engine: OpenMP threads (0 = all cores)
    size_t hybrid_cpu_threads = 0;

    std::string state_dir;
    bool resume = false;

    std::string output_path;                         // finalize() writes the result there as GeoTIFF (pcr/io/grid_io.h)
    bool write_cog = false;                          // with overview levels (GeoTiffOptions::overviews = -1); the HIP engine
                                                     // builds them in HBM and copies only the levels out

    // ---- extensions (not in the reference; defaults keep reference behaviour) ----------
    MemoryLocation result_location = MemoryLocation::Host;   // Device: finalize() leaves bands in HBM
    // Row-block sharding of the grid over GPUs: this pipeline ingests points whose centre row
    // is in [shard_row_begin, shard_row_end) and finalizes those rows; -1 = whole grid.
    int shard_row_begin = -1;
    int shard_row_end = -1;
    // Rows of state kept beyond each side of the owned block (glyph footprints of points near the block edge land
    // there and are sent to the owning rank).  -1: sized from the glyph defaults (Gaussian: max_radius_cells; Line:
    // default_half_length / |cell_size_y|, which max_radius_cells does NOT cap on north-up grids).  A Line glyph with a
    // per-point half_length channel can reach further: ingest() checks every cloud and refuses (InvalidArgument,
    // naming the rows needed) rather than clip silently -- raise this knob then.  Same value on every rank.
    int shard_halo_rows = -1;
    int scatter_path = 0;                            // 0 auto, 1 direct atomics, 2 binned LDS tiles, 3 moments+convolution (Gaussian)
    // The first Point scatter of a pipeline also stores the finished bands (they are dropped again by any later ingest): the
    // right default when finalize() follows a single ingest; pipelines that always ingest several clouds save one wasted band
    // store by switching it off.
    bool finalize_with_first_ingest = true;
    // 1..32: finalize() fills the NaN cells of the Average, WeightedAverage, Min, Max and MostRecent bands from their valid
    // neighbours within this many cells (pcr/core/fill_nodata.h); Sum and Count bands stay as they are.  result(), the
    // written GeoTIFF and its overview levels hold the filled bands; the accumulation state is untouched.  0: nothing is
    // allocated or launched.  A row-block shard lacks its neighbours' rows and refuses it (fill the gathered grid).
    int fill_nodata_radius = 0;
    // ground.source_band names an output band: finalize() appends a DTM band -- that band with its non-ground cells removed
    // (NaN) -- and, with ground.top_band, a height-above-ground band, top - DTM.  The filter reads the RAW source band, the
    // measured minima; with fill_nodata_radius the DTM is then filled like a Min band (filling never chains: a removed
    // building wider than twice the radius keeps a NaN core) and hag is taken from the bands as they leave the pipeline,
    // filled.  result(), the GeoTIFF and its overview levels carry the new bands as ordinary bands; the accumulation state
    // is untouched.  Empty source_band: nothing is allocated or launched.  A row-block shard refuses it.
    GroundFilterConfig ground;
    // Terrain bands: finalize() appends, behind the ground filter's bands and in list order, one band per entry -- a product of
    // pcr/core/terrain.h of the named band AS IT LEAVES the pipeline (filled: a hillshade of the filled DTM is the product
    // wanted), with the grid's signed cell sizes.  The new bands are never filled themselves.  Entries that share source,
    // z_factor and compute_edges cost one sweep over the source.  result(), the GeoTIFF and its overview levels carry them as
    // ordinary bands ("average" overviews of an aspect band are not meaningful near north); the accumulation state is
    // untouched.  Empty: nothing is allocated or launched.  A row-block shard refuses it.
    std::vector<TerrainBandConfig> terrain;
    // Individual trees: finalize() appends, behind the terrain bands and in list order, two bands per entry -- tree_id and
    // tree_height of pcr/core/trees.h of the named band AS IT LEAVES the pipeline (filled), with the grid's cell sizes; the
    // canopy height model is a Max of a "hag" surface channel.  The new bands are never filled.  A source is any reduction,
    // percentile, extremes or cell-stats band, the DTM or the hag band; terrain and tree bands are none.  result(), the GeoTIFF
    // and its overview levels carry the bands as ordinary bands ("average" overviews of an id band are not meaningful);
    // Pipeline::trees reads an entry's table.  The accumulation state is untouched.  create() refuses more than 4 entries, an
    // unknown source, a band name that collides with any other leaving band, a parameter outside its range and a row-block
    // shard, each naming the entry.  Empty: nothing is allocated, launched or validated differently.
    std::vector<TreeBandConfig> trees;
    // ingest_file of a LAS file: subtracted from the GPS time, in Float64, before it becomes the Float32 `gps_time` channel
    // (LasOptions::gps_time_origin; a MostRecent timestamp needs it: Float32 resolves 32 s at 3e8 s).
    double las_gps_time_origin = 0.0;
    // Surface channels: per-point channels derived from a band at every ingest (every chunk of ingest_file), after the
    // reprojection -- the reprojected coordinates are sampled, so the surface is in the grid's CRS -- and before the filters,
    // which may test them.  A name works wherever the configuration names a Float32 channel: a reduction's value_channel or
    // timestamp_channel, a glyph's per-point channels, a predicate of `filter` or of a ReductionSpec::filter ("hag > 2").  A
    // NaN sample (a point outside the surface, over a NaN cell, with a NaN value) is a NaN channel value like one a cloud
    // brings: reductions treat it as they do, every predicate on it but NotEqual and NotInSet is false.  On the HIP engine the channel is gathered in
    // HBM on the pipeline's stream -- ingest_file of a LAS tile still ships raw records -- and a configuration gives the same
    // channel bits on both engines.  Each name needs its surface before the first ingest (Pipeline::set_surface); checkpoints
    // record no surface.  create() refuses an empty or duplicate name, a value_channel that is itself a surface channel, more
    // than 8 entries, a row-block shard and a pipeline that has to run out of core.  Empty: nothing is allocated, launched or
    // validated differently.
    std::vector<SurfaceChannelConfig> surface_channels;
    // Per-point Float32 channels derived at ingest from polygons (PolygonChannelConfig, pcr/core/polygons.h: the exact per-point
    // test): at every ingest and every chunk of ingest_file, after reprojection and beside the surface channels, before the
    // filters, each point gets the value of the greatest-index polygon that holds it -- the exact clip (a filter on the name)
    // and the exact tag ("which plot").  The name works wherever a Float32 channel is named.  On the HIP engine the index
    // tables live in HBM the pipeline owns and the kernel runs on the pipeline's stream with no host wait; the host engine runs
    // the twin and gives the same channel bits.  Each name needs its polygons before the first ingest
    // (Pipeline::set_polygons); checkpoints record no polygons.  create() refuses an empty or duplicate name, a name that is
    // also a surface channel, more than 8 entries, a row-block shard and a pipeline that has to run out of core.  Empty: nothing
    // is allocated, launched or validated differently.
    std::vector<PolygonChannelConfig> polygon_channels;
    // Per-cell histograms (HistogramConfig): every ingest also counts each entry's channel into its cube -- on the HIP engine
    // in HBM, bins * cells * 4 bytes that count towards gpu_memory_budget -- and finalize() appends its percentile bands BEHIND
    // the reductions' bands and AHEAD of the DTM, hag and terrain bands: with fill_nodata_radius they are filled like a Max
    // band, ground.source_band, ground.top_band and terrain[].source_band may name them, result(), the GeoTIFF and its
    // overview levels carry them like any other band.  The cube persists like the plane state: finalize() may be called again
    // after more ingests; Pipeline::histogram_counts reads it at any time.  Each filter joins the plan of the ReductionSpec
    // filters and counts against its limits (8 distinct filters, 16 predicates per conjunction, 32 in all).  create() refuses
    // more than 4 entries, bins outside 1..256, non-finite bounds or lo >= hi, more than 16 percentiles, a percentile outside
    // [0, 1] or NaN, an empty value_channel, band_names longer than percentiles, a band name that collides with any other
    // leaving band, a row-block shard and a pipeline that has to run out of core; save_state, load_state and resume answer
    // NotImplemented while the list is non-empty (a checkpoint that silently lost the cube would be a wrong result later).
    // Empty: nothing is allocated, launched or validated differently.
    std::vector<HistogramConfig> histograms;
    // Per-cell extremes (ExtremesConfig): every ingest also folds each entry's channel into its k key planes -- on the HIP
    // engine in HBM, k * cells * 4 bytes that count towards gpu_memory_budget -- and finalize() appends one band per entry
    // BEHIND the percentile bands and AHEAD of the DTM, hag and terrain bands: with fill_nodata_radius it is filled like a Min
    // band (Lowest) or a Max band (Highest), ground.source_band, ground.top_band and terrain[].source_band may name it (a DTM
    // from "z_low" starts from outlier-free minima), result(), the GeoTIFF and its overview levels carry it like any other
    // band.  The planes persist like the plane state: finalize() may be called again after more ingests;
    // Pipeline::extremes_values reads them at any time.  Each filter joins the plan of the ReductionSpec filters and counts
    // against its limits (8 distinct filters, 16 predicates per conjunction, 32 in all).  create() refuses more than 4 entries,
    // k outside 2..8, a negative or NaN max_gap, an empty value_channel, an unknown side, a band name that collides with any
    // other leaving band, a row-block shard and a pipeline that has to run out of core; save_state, load_state and resume
    // answer NotImplemented while the list is non-empty.  Empty: nothing is allocated, launched or validated differently.
    std::vector<ExtremesConfig> extremes;
    // Per-cell stats (CellStatsConfig): every ingest also folds each entry's channel into its three integer planes -- on the HIP
    // engine in HBM, 20 bytes per cell that count towards gpu_memory_budget -- and finalize() appends one band per product
    // BEHIND the extremes' bands and AHEAD of the DTM, hag and terrain bands.  With fill_nodata_radius a Mean band is filled like
    // an Average band; Variance and StdDev bands are never filled (a spread made up from the neighbours' is no measurement).
    // ground.source_band, ground.top_band and terrain[].source_band may name the bands ("z_mean"); result(), the GeoTIFF and its
    // overview levels carry them like any other band.  The planes persist like the plane state: finalize() may be called again
    // after more ingests; Pipeline::cell_stats_state reads them at any time.  Each filter joins the plan of the ReductionSpec
    // filters and counts against its limits.  create() refuses more than 4 entries, an empty value_channel, a resolution that is
    // not finite and positive (or whose reciprocal is not finite), a non-finite origin, products empty, longer than 3 or with a
    // duplicate, ddof other than 0 or 1, band_names longer than products, a band name that collides with any other leaving
    // band, a row-block shard and a pipeline that has to run out of core; save_state, load_state and resume answer
    // NotImplemented while the list is non-empty.  Empty: nothing is allocated, launched or validated differently.
    std::vector<CellStatsConfig> cell_stats;
    // Zonal tables (ZonalConfig): Pipeline::zonal(i) folds the chosen cell-stats planes and histogram cubes by entry i's label band
    // into one row per zone -- on the HIP engine in HBM, only the table crosses PCIe.  Nothing happens at ingest or in finalize()
    // and no band is added.  create() refuses more than 4 entries, an empty `zones`, a `zones` that names no band of the result
    // unless `external` is set, an index outside cell_stats or histograms, more than 16 percentiles or one outside [0, 1], a
    // column name that appears twice, max_zones outside 1..2^24, a row-block shard and a pipeline that has to run out of core.
    // Empty: nothing is allocated, launched or validated differently.
    std::vector<ZonalConfig> zonal;
    // Point zonal tables (PointZonalConfig): at every ingest, and every chunk of ingest_file, each entry's specs are folded by its
    // label channel into one row per zone, after the derived channels and the filter classes -- on the HIP engine in HBM on the
    // pipeline's stream, max_zones * (8 + 24 * stats + 8 * sum of bins) bytes per entry that are allocated at create and count
    // towards gpu_memory_budget; only the table crosses PCIe.  The grid plays no part: a point outside it counts.
    // Pipeline::point_zonal(i) reads the table at any time; finalize() neither needs nor changes it.  Each spec's filter joins the
    // plan of the ReductionSpec filters and counts against its limits.  ingest_file decodes a LAS channel that only an entry here
    // names.  create() refuses more than 4 entries, more than 4 stats specs or 4 histograms in one, an empty label_channel, a
    // column name that appears twice, max_zones outside 1..2^24, what PipelineConfig::cell_stats and ::histograms refuse about a
    // spec's own fields, a row-block shard and a pipeline that has to run out of core; save_state, load_state and resume answer
    // NotImplemented while the list is non-empty.  Empty: nothing is allocated, launched or validated differently.
    std::vector<PointZonalConfig> point_zonal;
};

struct ProgressInfo {
    size_t collections_processed = 0;
    size_t collections_total = 0;
    size_t points_processed = 0;
    size_t tiles_active = 0;
    float elapsed_seconds = 0.0f;
};

using ProgressCallback = std::function<bool(const ProgressInfo& info)>;

class Pipeline {
public:
    ~Pipeline();

    static std::unique_ptr<Pipeline> create(const PipelineConfig& config);   // nullptr on failure

    Status validate() const;
    Status ingest(const PointCloud& cloud);
    /// Extension: like ingest, but returns once the work is enqueued when the cloud is
    /// page-locked (HostPinned) or device-resident; the cloud must stay untouched until synchronize() /
    /// finalize().  Pageable host clouds behave as in ingest.
    Status ingest_async(const PointCloud& cloud);
    /// Extension: streams a PCRP / CSV / LAS file through two page-locked chunk buffers -- the file read of chunk
    /// k+1 overlaps the host-to-device copy and the kernels of chunk k.  `points_read` (optional) = rows read.
    /// LAS: only the channels the configuration names (reductions, glyphs, filter) are decoded -- one the file's point
    /// format lacks is InvalidArgument; on the HIP engine the raw records cross PCIe and are unpacked in HBM.
    Status ingest_file(const std::string& path, size_t chunk_points = 4u << 20, size_t* points_read = nullptr);
    /// Extension: gives the surface channel `name` (PipelineConfig::surface_channels) its surface -- band `band` of `grid`,
    /// which carries its geometry (Grid::set_geometry; result() of another pipeline over a whole grid does) and need not be
    /// this pipeline's grid.  The band and the geometry are copied into memory the pipeline owns (HBM on the HIP engine), so
    /// the caller's grid may die or change afterwards; a Device grid's band must be complete (after finalize(), or
    /// finalize_async() + synchronize()).  May be called again between ingests; on the HIP engine it waits for the pipeline's
    /// stream first.  InvalidArgument for an unknown name, a grid without geometry, a band outside the grid or not Float32;
    /// CrsError when the surface's CRS and the grid's are both identified and differ.
    Status set_surface(const std::string& name, const Grid& grid, int band = 0);
    /// Extension: gives the polygon channel `name` (PipelineConfig::polygon_channels) its polygons, in the CRS of the pipeline's
    /// grid.  The index is built on the host and kept (on the HIP engine its tables are uploaded once, into HBM the pipeline
    /// owns, after waiting for the pipeline's stream), so the caller's set may die or change afterwards; it may be called again
    /// between ingests.  InvalidArgument for an unknown name (which a sharded or out-of-core pipeline has none of) and for what
    /// points_in_polygons refuses about the set and the options.
    Status set_polygons(const std::string& name, const PolygonSet& polygons,
                        const PointInPolygonOptions& options = PointInPolygonOptions());
    /// Extension: the cube of PipelineConfig::histograms[i] as a host copy, [bins][rows][width] counters, after synchronising
    /// with the pipeline's stream.  Valid after any ingest (all zero before the first); finalize() is not needed.  Height strata
    /// and canopy cover above any threshold are sums of its bin planes.  InvalidArgument for an index outside the list.
    Status histogram_counts(int i, std::vector<uint32_t>* out) const;
    /// ... and its shape: bins planes of rows x width cells.
    Status histogram_shape(int i, int* bins, int* rows, int* width) const;
    /// Extension: the values PipelineConfig::extremes[i] keeps as a host copy, [k][rows][width] floats -- ascending for Lowest,
    /// descending for Highest, NaN for an empty slot -- after synchronising with the pipeline's stream.  Valid after any ingest
    /// (all NaN before the first); finalize() is not needed.  InvalidArgument for an index outside the list.
    Status extremes_values(int i, std::vector<float>* out) const;
    /// ... and its shape: k planes of rows x width cells.
    Status extremes_shape(int i, int* k, int* rows, int* width) const;
    /// Extension: the three planes of PipelineConfig::cell_stats[i] as host copies, rows x width each -- N, S1 (the sum of the
    /// steps) and S2 (the sum of their squares) -- after synchronising with the pipeline's stream.  Valid after any ingest (all
    /// zero before the first); finalize() is not needed.  InvalidArgument for an index outside the list.
    Status cell_stats_state(int i, std::vector<uint32_t>* n, std::vector<int64_t>* s1, std::vector<uint64_t>* s2) const;
    /// ... and its shape.
    Status cell_stats_shape(int i, int* rows, int* width) const;
    /// Extension: the table of PipelineConfig::trees[i] as the last finalize() left it -- one row per tree, ids 1..size(), the
    /// cell centres by the grid's geometry.  Valid after a finalize (also finalize_async: on the HIP engine the call waits for
    /// the pipeline's stream and fetches the table then); a later finalize replaces it, and nothing else does: after further
    /// ingests the table is still the last finalize's, like result().  InvalidArgument for an index outside
    /// the list or before the first finalize; OutOfRange for more than 2^24 trees.
    Status trees(int i, TreeTable* out) const;
    /// Extension: gives the external label grid `name` (a PipelineConfig::zonal entry with `external`) its labels -- band `band`
    /// of `grid`, which must have the pipeline's width and height.  The band is copied into memory the pipeline owns (HBM on
    /// the HIP engine: a Host grid is uploaded, a Device grid copied in place on the device), so the caller's grid may die or
    /// change afterwards.  InvalidArgument for an unknown name, another shape, a band outside the grid or not Float32.
    Status set_zones(const std::string& name, const Grid& grid, int band = 0);
    /// Extension: the same with the labels burnt from polygons on PipelineConfig::grid (pcr/core/polygons.h: the cell-centre
    /// rule, the greatest index wins, p + 1 or `values`): a plot or stand map straight from its outlines.  On the HIP engine the
    /// polygons are scan-converted in HBM on the pipeline's stream, into memory the pipeline owns; on the host engine by the host
    /// twin, bit for bit the same band.  InvalidArgument for an unknown name (which a sharded or out-of-core pipeline has
    /// none of) and for what rasterize_polygons refuses.
    Status set_zones(const std::string& name, const PolygonSet& polygons, const RasterizeOptions& options = RasterizeOptions());
    /// Extension: the table of PipelineConfig::zonal[i] -- the zone band as the last finalize() left it (or the external grid),
    /// the cell-stats planes and cubes as they are.  Valid after a finalize with no ingest since -- an ingest of an empty cloud, or
    /// of one that PipelineConfig::filter keeps no point of, changes no state and does not count, on either engine; handing out or
    /// writing through state_planes() and the touched flags, merge_touched and a refused save_state / load_state leave the table
    /// as it is, as they leave Pipeline::trees' (also finalize_async: on the HIP
    /// engine the call is enqueued behind it on the pipeline's stream, which is waited for once for the number of zones and once
    /// for the table).  InvalidArgument for an index outside the list, before the first finalize, after a further ingest or for
    /// an external grid that was not set; OutOfRange for a zone above the entry's max_zones.  with_counts: also copy out every
    /// histogram's [zone][bin] counts (HistColumns::counts; zones x bins x 8 bytes each), which are left empty otherwise.
    Status zonal(int i, ZonalTable* out, bool with_counts = false) const;
    /// Extension: the table of PipelineConfig::point_zonal[i] as the ingests so far left it -- valid after any ingest (no row before
    /// the first), finalize() is not needed and does not change it.  On the HIP engine the rows are made in HBM behind everything
    /// on the pipeline's stream, which is waited for once for the info words and once for the table.  InvalidArgument for an
    /// index outside the list; OutOfRange while the overflow counter is nonzero (a kept point carried a zone above max_zones).
    /// with_counts: also copy out every histogram's [zone][bin] counts.
    Status point_zonal(int i, PointZonalTable* out, bool with_counts = false) const;
    /// Extension: the zones of the result's band `band_name` as polygons on PipelineConfig::grid (pcr/core/polygons.h: polygonize)
    /// -- the crowns of a "..._tree_id" band, whose polygon of value z belongs to row z - 1 of zonal(i) and trees(i).  The set
    /// comes from the band as the last finalize() left it and is valid under zonal(i)'s condition: after a finalize with no ingest
    /// since.  On the HIP engine it is made in HBM behind everything on the pipeline's stream, in work areas of the call's own, and
    /// only the ring table crosses PCIe; the host engine runs the host twin: the same set bit for bit.  InvalidArgument for a name
    /// that is no Float32 band of the result, before the first finalize, after a further ingest, for a row-block shard and for an
    /// out-of-core pipeline.
    Status polygonize(const std::string& band_name, PolygonSet* out) const;
    Status finalize();
    /// Extension, the counterpart of ingest_async: with a device-resident result (result_location = Device, no output_path)
    /// the finalize kernels are only ENQUEUED on the pipeline's stream -- result() is valid at once, its bands are complete
    /// after synchronize() (or for anything ordered after it on stream_handle()).  Back-to-back pipelines then never leave
    /// the device idle for a host round trip.  Any other configuration behaves as finalize().
    Status finalize_async();
    Status run(const std::vector<const PointCloud*>& clouds);
    void set_progress_callback(ProgressCallback cb);
    const Grid* result() const;
    ProgressInfo stats() const;

    // ---- checkpoint / resume in the reference's `.pcrt` tile-state format (pcr/io/tile_state_io.h).
    // save_state writes one file per touched reference tile and ReductionSpec (directly into `dir` for a
    // single reduction -- the reference's layout -- else into dir/reduction_<i>/); load_state sets the
    // device state from such files (also ones written by the reference) and marks their tiles touched.
    // An empty `dir` means PipelineConfig::state_dir.  PipelineConfig::resume = true loads at create().
    // Unlike the reference, finalize() never writes state files implicitly.
    Status save_state(const std::string& dir = "");
    Status load_state(const std::string& dir = "");

    // ---- extensions for row-block sharded runs (halo exchange is driven by the caller,
    //      e.g. torch.distributed over RCCL: see pcr/distributed.py) -------------------------
    struct PlaneView {
        void* device_ptr;      // first float of the plane (row state_row_begin)
        int plane_kind;        // PCR_HIP_PLANE_* of include/pcr_hip.h (a MostRecent group: a read-only snapshot of its value /
                               // timestamp planes in the SUM / WGT slots, refreshed by every state_planes() call)
        int group;             // accumulation group index
        int reach_rows;        // rows the group's glyph can reach beyond a point's centre row (0: Point glyph -- its halo
                               // rows never receive anything and need no exchange)
    };
    int halo_rows() const;                       // rows kept above/below the owned block
    // Row-block shards: rows the Line groups need beyond a centre row for this cloud (0: no check applies).  ingest()
    // refuses a cloud that needs more than halo_rows(); sharded callers agree on MAX over ranks first.
    Status line_reach_rows(const PointCloud& cloud, int* rows);
    int state_row_begin() const;
    int state_row_count() const;
    std::vector<PlaneView> state_planes() const;
    /// Accumulation group of every ReductionSpec, in order (the `group` of state_planes()); empty on the other engines.
    std::vector<int> reduction_groups() const;
    void* tile_touched_device(int* tiles_x, int* tiles_y) const;
    /// The same flags for READING only (nothing is assumed to change: bands a scatter stored stay valid).
    const void* tile_touched_device_readonly(int* tiles_x, int* tiles_y) const;
    /// Row-block shards: ORs `d_union` (tiles_x * tiles_y device words: the all-reduced flags of every rank) into this
    /// pipeline's flags on its stream; bands a scatter stored are dropped -- on the device -- only when a flag really changed.
    Status merge_touched(const void* d_union);
    /// The finished band `band` of the last finalize() in DEVICE memory (own rows x width floats; the device-resident
    /// result's band, or the device-side copy a host-resident result was made from): what a sharded gather sends.
    /// nullptr before the first finalize, out of core, or for a band index outside the result.
    const float* result_band_device(int band) const;
    Status synchronize();
    void* stream_handle() const;                 // the hipStream_t every kernel of this pipeline runs on (may be null)
    // per-kernel HIP-event timing of the scatter kernels (roofline reporting)
    struct KernelTime { std::string name; unsigned launches; double total_ms; };
    void profile_enable(bool on, const std::string& only_kernel = "");   // only_kernel: bracket just that kernel with events
    std::vector<KernelTime> profile_read(bool reset);
    // path and LDS tiling the last scatter used (0 direct, 1 binned), exact valid-point count
    // bands_with_scatter: accumulation groups whose finished bands the scatter that defined their planes was asked to store
    // too and that nothing has invalidated since (finalize skips their kernel when the device confirms)
    // deferred_planes: plane bits (1 Sum, 2 Count, 4 Max, 8 Min) that scatter was let off storing, their values being in the
    // band of their own reduction; they are put back, once, in front of whatever next reads or changes the state
    struct ScatterInfo { int path; int lds_tile_w, lds_tile_h, lds_apron, num_bins; size_t points_in, points_valid; int scatter_chunk; int bands_with_scatter; int deferred_planes; };
    ScatterInfo last_scatter() const;

    /// True when the grid's state did not fit the device budget and the pipeline sweeps it in row bands (out of core).
    bool out_of_core() const;
    /// Out of core: the pipeline's own directory of evicted bands -- `.pcrt` tile files in the reference's layout, removed with
    /// the pipeline (save_state() writes checkpoints that stay).  Empty otherwise.
    std::string spill_dir() const;
    /// "hip" (the MI355X engine) or "host" (ExecutionMode::CPU, or a fallback the reference would have taken too).
    const char* engine() const;
    /// OpenMP threads of the host engine (cpu_threads, or every CPU the process may use: affinity and cgroup quota); 0 on "hip".
    int host_threads() const;

private:
    Pipeline() = default;
    Status ingest_las_records(const std::string& path, const LasOptions& options, size_t chunk_points, size_t* points_read);
    struct Impl;
    struct Banded;                       // out-of-core driver: row bands of whole reference-tile rows, one in HBM at a time
    struct Host;                         // the pipeline on the host engine (host/src/host_pipeline.h)
    std::unique_ptr<Impl> impl_;
    std::unique_ptr<Banded> banded_;
    std::unique_ptr<Host> host_;
};

/// Extension: PointZonalConfig for any cloud, where it lives: a Device cloud is folded in HBM by the kernels (on the default stream,
/// which is waited for), a Host or HostPinned cloud by the host twins; the same bits either way.  No filter is applied: a spec
/// with a non-empty filter is InvalidArgument (filters are a pipeline's).  What Pipeline::create refuses about an entry is
/// InvalidArgument here, a missing or non-Float32 channel too; OutOfRange for a zone above max_zones.
Status point_zonal(const PointCloud& cloud, const PointZonalConfig& config, PointZonalTable* out, bool with_counts = false);

// Why the last Pipeline::create() on this thread returned nullptr.
const std::string& pipeline_create_error();

}  // namespace pcr
