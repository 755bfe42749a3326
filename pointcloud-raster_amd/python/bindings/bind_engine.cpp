// bind_engine.cpp -- FilterSpec, GlyphSpec, ReductionSpec, PipelineConfig, ProgressInfo, Pipeline.
#include "common.h"

#include "pcr/core/grid.h"
#include "pcr/core/point_cloud.h"
#include "pcr/engine/filter.h"
#include "pcr/engine/glyph.h"
#include "pcr/engine/pipeline.h"
#include "pcr/engine/sharded_pipeline.h"
#include "../../host/src/ground_filter.h"
#include "../../host/src/terrain.h"
#include "../../host/src/zone_rows.h"

using namespace pcr;

namespace {

// Pipeline.zonal's, Pipeline.point_zonal's and pcr.point_zonal's dict: the columns of zone_rows.h, `count` as "cells" or "points".
py::dict zone_dict(const std::vector<int32_t>& zone, const char* count_name, const std::vector<int64_t>& count,
                   const std::vector<ZonalTable::StatColumns>& stats, const std::vector<ZonalTable::HistColumns>& hists) {
    py::dict d;
    detail::for_each_zone_column(zone, count_name, count, stats, hists, [&d](const std::string& name, const auto& v) {
        using T = typename std::decay_t<decltype(v)>::value_type;
        py::array_t<T> a((py::ssize_t)v.size());
        if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
        d[py::str(name)] = a;
    });
    return d;
}
py::dict point_zonal_dict(const PointZonalTable& t) { return zone_dict(t.zone, "points", t.points, t.stats, t.hists); }

// Pipeline.zonal_histogram's and Pipeline.point_zonal_histogram's array: the (zones, bins) counts of the h-th histogram.
py::array_t<uint64_t> zone_histogram(const char* fn, size_t zones, const std::vector<ZonalTable::HistColumns>& hists, int h) {
    if (h < 0 || (size_t)h >= hists.size())
        throw std::runtime_error(std::string("pipeline: ") + fn + ": no histogram " + std::to_string(h) + " in the entry");
    const auto& c = hists[(size_t)h];
    py::array_t<uint64_t> a({(py::ssize_t)zones, (py::ssize_t)c.bins});
    if (!c.counts.empty()) std::memcpy(a.mutable_data(), c.counts.data(), c.counts.size() * sizeof(uint64_t));
    return a;
}

}  // namespace

void bind_engine(py::module_& m) {
    py::enum_<ExecutionMode>(m, "ExecutionMode")
        .value("CPU", ExecutionMode::CPU).value("GPU", ExecutionMode::GPU)
        .value("Auto", ExecutionMode::Auto).value("Hybrid", ExecutionMode::Hybrid).export_values();

    py::enum_<CompareOp>(m, "CompareOp")
        .value("Equal", CompareOp::Equal).value("NotEqual", CompareOp::NotEqual)
        .value("Less", CompareOp::Less).value("LessEqual", CompareOp::LessEqual)
        .value("Greater", CompareOp::Greater).value("GreaterEqual", CompareOp::GreaterEqual)
        .value("InSet", CompareOp::InSet).value("NotInSet", CompareOp::NotInSet).export_values();

    py::enum_<GlyphType>(m, "GlyphType")
        .value("Point", GlyphType::Point).value("Line", GlyphType::Line)
        .value("Gaussian", GlyphType::Gaussian).export_values();

    py::class_<FilterPredicate>(m, "FilterPredicate")
        .def(py::init<>())
        .def_readwrite("channel_name", &FilterPredicate::channel_name)
        .def_readwrite("op", &FilterPredicate::op)
        .def_readwrite("value", &FilterPredicate::value)
        .def_readwrite("value_set", &FilterPredicate::value_set);

    py::class_<FilterSpec>(m, "FilterSpec")
        .def(py::init<>())
        .def_readwrite("predicates", &FilterSpec::predicates)
        .def("add", &FilterSpec::add, py::arg("channel"), py::arg("op"), py::arg("value"),
             py::return_value_policy::reference_internal)
        .def("add_in_set", &FilterSpec::add_in_set, py::arg("channel"), py::arg("values"),
             py::return_value_policy::reference_internal)
        .def("empty", &FilterSpec::empty);

    py::class_<GlyphSpec>(m, "GlyphSpec")
        .def(py::init<>())
        .def_readwrite("type", &GlyphSpec::type)
        .def_readwrite("direction_channel", &GlyphSpec::direction_channel)
        .def_readwrite("default_direction", &GlyphSpec::default_direction)
        .def_readwrite("half_length_channel", &GlyphSpec::half_length_channel)
        .def_readwrite("default_half_length", &GlyphSpec::default_half_length)
        .def_readwrite("sigma_x_channel", &GlyphSpec::sigma_x_channel)
        .def_readwrite("default_sigma_x", &GlyphSpec::default_sigma_x)
        .def_readwrite("sigma_y_channel", &GlyphSpec::sigma_y_channel)
        .def_readwrite("default_sigma_y", &GlyphSpec::default_sigma_y)
        .def_readwrite("rotation_channel", &GlyphSpec::rotation_channel)
        .def_readwrite("default_rotation", &GlyphSpec::default_rotation)
        .def_readwrite("max_radius_cells", &GlyphSpec::max_radius_cells)
        .def_readwrite("normalize_weights", &GlyphSpec::normalize_weights)
        .def("__repr__", [](const GlyphSpec& g) {
            static const char* names[] = {"Point", "Line", "Gaussian"};
            return std::string("GlyphSpec(type=") + names[static_cast<int>(g.type)] + ")";
        });

    py::class_<ReductionSpec>(m, "ReductionSpec")
        .def(py::init<>())
        .def_readwrite("value_channel", &ReductionSpec::value_channel)
        .def_readwrite("type", &ReductionSpec::type)
        .def_readwrite("weight_channel", &ReductionSpec::weight_channel)
        .def_readwrite("timestamp_channel", &ReductionSpec::timestamp_channel,
                       "ReductionType.MostRecent (Point glyph only): the Float32 channel whose greatest value picks the cell's point "
                       "(\"newest survey wins\"). Points with a NaN or <= -FLT_MAX timestamp are ignored; among equal timestamps the "
                       "greater value wins, so the result does not depend on order, engine or chunking. Required for MostRecent.")
        .def_readwrite("percentile", &ReductionSpec::percentile)
        .def_readwrite("output_band_name", &ReductionSpec::output_band_name)
        .def_readwrite("glyph", &ReductionSpec::glyph)
        .def_readwrite("filter", &ReductionSpec::filter,
                       "This reduction folds only the points that pass PipelineConfig.filter AND this FilterSpec (empty: every "
                       "survivor of the pipeline's filter). spec.filter.add(...) works in place. The touched-tile flags come from "
                       "PipelineConfig.filter's survivors alone: a filtered Sum is 0, not NaN, in a tile other points touched.");

    py::class_<GroundFilterConfig, GroundFilterSpec>(m, "GroundFilterConfig")
        .def(py::init<>())
        .def(py::init<const GroundFilterConfig&>())
        .def_readwrite("source_band", &GroundFilterConfig::source_band)
        .def_readwrite("top_band", &GroundFilterConfig::top_band)
        .def_readwrite("dtm_band_name", &GroundFilterConfig::dtm_band_name)
        .def_readwrite("hag_band_name", &GroundFilterConfig::hag_band_name);

    py::class_<TerrainBandConfig, TerrainSpec>(m, "TerrainBandConfig")
        .def(py::init<>())
        .def(py::init<const TerrainBandConfig&>())
        .def_readwrite("source_band", &TerrainBandConfig::source_band)
        .def_readwrite("product", &TerrainBandConfig::product)
        .def_readwrite("band_name", &TerrainBandConfig::band_name);

    py::class_<TreeBandConfig, TreeSpec>(m, "TreeBandConfig",
                                         "The tree_id and tree_height bands of one band of the result, appended at finalize()")
        .def(py::init<>())
        .def(py::init<const TreeBandConfig&>())
        .def(py::init([](const std::string& source_band, const std::string& id_band_name, const std::string& height_band_name) {
            TreeBandConfig c;
            c.source_band = source_band;
            c.id_band_name = id_band_name;
            c.height_band_name = height_band_name;
            return c;
        }), py::arg("source_band"), py::arg("id_band_name") = "", py::arg("height_band_name") = "")
        .def_readwrite("source_band", &TreeBandConfig::source_band)
        .def_readwrite("id_band_name", &TreeBandConfig::id_band_name)
        .def_readwrite("height_band_name", &TreeBandConfig::height_band_name);

    py::class_<SurfaceChannelConfig>(m, "SurfaceChannelConfig")
        .def(py::init<>())
        .def(py::init<const SurfaceChannelConfig&>())
        .def(py::init([](const std::string& name, const std::string& value_channel, SampleMode mode) {
            SurfaceChannelConfig c;
            c.name = name;
            c.value_channel = value_channel;
            c.mode = mode;
            return c;
        }), py::arg("name"), py::arg("value_channel") = "", py::arg("mode") = SampleMode::Bilinear)
        .def_readwrite("name", &SurfaceChannelConfig::name)
        .def_readwrite("value_channel", &SurfaceChannelConfig::value_channel)
        .def_readwrite("mode", &SurfaceChannelConfig::mode);

    py::class_<PolygonChannelConfig>(m, "PolygonChannelConfig",
                                     "One entry of PipelineConfig.polygon_channels: the Float32 channel `name`, derived at every ingest from "
                                     "the polygons given with Pipeline.set_polygons -- the value of the polygon that holds the point, exactly")
        .def(py::init<>())
        .def(py::init<const PolygonChannelConfig&>())
        .def(py::init([](const std::string& name) {
            PolygonChannelConfig c;
            c.name = name;
            return c;
        }), py::arg("name"))
        .def_readwrite("name", &PolygonChannelConfig::name);

    py::class_<HistogramConfig>(m, "HistogramConfig",
                                "One per-cell histogram of a Float32 channel (a surface channel included) and its percentile bands")
        .def(py::init<>())
        .def(py::init<const HistogramConfig&>())
        .def(py::init([](const std::string& value_channel, float lo, float hi, int bins, const std::vector<float>& percentiles) {
            HistogramConfig h;
            h.value_channel = value_channel;
            h.lo = lo;
            h.hi = hi;
            h.bins = bins;
            h.percentiles = percentiles;
            return h;
        }), py::arg("value_channel"), py::arg("lo") = 0.0f, py::arg("hi") = 64.0f, py::arg("bins") = 32,
            py::arg("percentiles") = std::vector<float>())
        .def_readwrite("value_channel", &HistogramConfig::value_channel)
        .def_readwrite("lo", &HistogramConfig::lo)
        .def_readwrite("hi", &HistogramConfig::hi)
        .def_readwrite("bins", &HistogramConfig::bins)
        .def_readwrite("filter", &HistogramConfig::filter)
        .def_readwrite("percentiles", &HistogramConfig::percentiles)
        .def_readwrite("band_names", &HistogramConfig::band_names);

    py::enum_<ExtremeSide>(m, "ExtremeSide")
        .value("Lowest", ExtremeSide::Lowest)
        .value("Highest", ExtremeSide::Highest);

    py::class_<ExtremesConfig>(m, "ExtremesConfig",
                               "The k lowest (or highest) distinct values of a Float32 channel per cell (a surface channel included) "
                               "and the outlier-free Min (Max) band walked out of them")
        .def(py::init<>())
        .def(py::init<const ExtremesConfig&>())
        .def(py::init([](const std::string& value_channel, ExtremeSide side, int k, float max_gap) {
            ExtremesConfig e;
            e.value_channel = value_channel;
            e.side = side;
            e.k = k;
            e.max_gap = max_gap;
            return e;
        }), py::arg("value_channel"), py::arg("side") = ExtremeSide::Lowest, py::arg("k") = 4, py::arg("max_gap") = 1.0f)
        .def_readwrite("value_channel", &ExtremesConfig::value_channel)
        // (an integer is taken as it is, so that a configuration written elsewhere with a side this build does not know is
        // refused by Pipeline.create with its message, not by the setter)
        .def_property("side", [](const ExtremesConfig& e) { return e.side; },
                      [](ExtremesConfig& e, const py::object& side) {
                          e.side = py::isinstance<ExtremeSide>(side) ? side.cast<ExtremeSide>() : static_cast<ExtremeSide>(side.cast<int>());
                      })
        .def_readwrite("k", &ExtremesConfig::k)
        .def_readwrite("max_gap", &ExtremesConfig::max_gap)
        .def_readwrite("filter", &ExtremesConfig::filter)
        .def_readwrite("band_name", &ExtremesConfig::band_name);

    py::enum_<CellStat>(m, "CellStat")
        .value("Mean", CellStat::Mean)
        .value("Variance", CellStat::Variance)
        .value("StdDev", CellStat::StdDev);

    py::class_<CellStatsConfig>(m, "CellStatsConfig",
                                "The exact mean, variance and standard deviation of a Float32 channel per cell (a surface channel "
                                "included), from integer sums of the value quantized to a step")
        .def(py::init<>())
        .def(py::init<const CellStatsConfig&>())
        .def(py::init([](const std::string& value_channel, double origin, double resolution, const std::vector<CellStat>& products, int ddof) {
            CellStatsConfig c;
            c.value_channel = value_channel;
            c.origin = origin;
            c.resolution = resolution;
            c.products = products;
            c.ddof = ddof;
            return c;
        }), py::arg("value_channel"), py::arg("origin") = 0.0, py::arg("resolution") = 0.01,
            py::arg("products") = std::vector<CellStat>{CellStat::StdDev}, py::arg("ddof") = 0)
        .def_readwrite("value_channel", &CellStatsConfig::value_channel)
        .def_readwrite("origin", &CellStatsConfig::origin)
        .def_readwrite("resolution", &CellStatsConfig::resolution)
        .def_readwrite("products", &CellStatsConfig::products)
        .def_readwrite("ddof", &CellStatsConfig::ddof)
        .def_readwrite("filter", &CellStatsConfig::filter)
        .def_readwrite("band_names", &CellStatsConfig::band_names);

    py::class_<ZonalConfig>(m, "ZonalConfig",
                            "One table with a row per zone -- per tree with a tree_id band, per plot with a label grid of "
                            "Pipeline.set_zones -- of the chosen cell_stats entries and histograms (Pipeline.zonal)")
        .def(py::init<>())
        .def(py::init<const ZonalConfig&>())
        .def(py::init([](const std::string& zones, bool external, const std::vector<int>& cell_stats, const std::vector<int>& histograms,
                         const py::object& percentiles, int max_zones) {
            ZonalConfig c;
            c.zones = zones;
            c.external = external;
            c.cell_stats = cell_stats;
            c.histograms = histograms;
            c.own_percentiles = percentiles.is_none();
            if (!c.own_percentiles) c.percentiles = percentiles.cast<std::vector<float>>();
            c.max_zones = max_zones;
            return c;
        }), py::arg("zones"), py::arg("external") = false, py::arg("cell_stats") = std::vector<int>{},
            py::arg("histograms") = std::vector<int>{}, py::arg("percentiles") = py::none(), py::arg("max_zones") = 1 << 22)
        .def_readwrite("zones", &ZonalConfig::zones)
        .def_readwrite("external", &ZonalConfig::external)
        .def_readwrite("cell_stats", &ZonalConfig::cell_stats)
        .def_readwrite("histograms", &ZonalConfig::histograms)
        .def_property("percentiles", [](const ZonalConfig& c) -> py::object {
            if (c.own_percentiles) return py::none();
            return py::cast(c.percentiles);
        }, [](ZonalConfig& c, const py::object& v) {
            c.own_percentiles = v.is_none();
            c.percentiles = c.own_percentiles ? std::vector<float>() : v.cast<std::vector<float>>();
        }, "None: every chosen histogram with its entry's own percentile list")
        .def_readwrite("max_zones", &ZonalConfig::max_zones);

    py::class_<PointZonalConfig>(m, "PointZonalConfig",
                                 "One table with a row per zone of a per-point label channel -- a polygon channel, a surface channel "
                                 "or the cloud's own -- of its own CellStatsConfig and HistogramConfig specs, folded at every ingest "
                                 "(Pipeline.point_zonal, pcr.point_zonal); the grid plays no part")
        .def(py::init<>())
        .def(py::init<const PointZonalConfig&>())
        .def(py::init([](const std::string& label_channel, const std::vector<CellStatsConfig>& cell_stats,
                         const std::vector<HistogramConfig>& histograms, int max_zones) {
            PointZonalConfig c;
            c.label_channel = label_channel;
            c.cell_stats = cell_stats;
            c.histograms = histograms;
            c.max_zones = max_zones;
            return c;
        }), py::arg("label_channel"), py::arg("cell_stats") = std::vector<CellStatsConfig>{},
            py::arg("histograms") = std::vector<HistogramConfig>{}, py::arg("max_zones") = 1 << 16)
        .def_readwrite("label_channel", &PointZonalConfig::label_channel)
        .def_readwrite("cell_stats", &PointZonalConfig::cell_stats)
        .def_readwrite("histograms", &PointZonalConfig::histograms)
        .def_readwrite("max_zones", &PointZonalConfig::max_zones);

    m.def("point_zonal", [](const PointCloud& cloud, const std::string& label_channel, const std::vector<CellStatsConfig>& cell_stats,
                            const std::vector<HistogramConfig>& histograms, int max_zones) {
        PointZonalConfig c;
        c.label_channel = label_channel;
        c.cell_stats = cell_stats;
        c.histograms = histograms;
        c.max_zones = max_zones;
        PointZonalTable t;
        Status s;
        {
            py::gil_scoped_release release;
            s = point_zonal(cloud, c, &t);
        }
        raise_if_error(s);
        return point_zonal_dict(t);
    }, py::arg("cloud"), py::arg("label_channel"), py::arg("cell_stats") = std::vector<CellStatsConfig>{},
       py::arg("histograms") = std::vector<HistogramConfig>{}, py::arg("max_zones") = 1 << 16,
          "PointZonalConfig's table for any cloud, where it lives: a Device cloud is folded in HBM, a Host cloud by the host twins; "
          "the same bits either way.  Spec filters are a pipeline's and are refused here");

    py::class_<PipelineConfig>(m, "PipelineConfig")
        .def(py::init<>())
        .def_readwrite("grid", &PipelineConfig::grid)
        .def_readwrite("reductions", &PipelineConfig::reductions)
        .def_readwrite("filter", &PipelineConfig::filter)
        .def_readwrite("target_crs", &PipelineConfig::target_crs)
        .def_readwrite("auto_reproject", &PipelineConfig::auto_reproject)
        .def_readwrite("exec_mode", &PipelineConfig::exec_mode)
        .def_readwrite("gpu_memory_budget", &PipelineConfig::gpu_memory_budget)
        .def_readwrite("host_cache_budget", &PipelineConfig::host_cache_budget)
        .def_readwrite("chunk_size", &PipelineConfig::chunk_size)
        .def_readwrite("cpu_threads", &PipelineConfig::cpu_threads)
        .def_readwrite("gpu_fallback_to_cpu", &PipelineConfig::gpu_fallback_to_cpu)
        .def_readwrite("hybrid_cpu_threads", &PipelineConfig::hybrid_cpu_threads)
        .def_readwrite("state_dir", &PipelineConfig::state_dir)
        .def_readwrite("resume", &PipelineConfig::resume)
        .def_readwrite("output_path", &PipelineConfig::output_path)
        .def_readwrite("write_cog", &PipelineConfig::write_cog)
        // fields the reference keeps C++-only, plus this build's extensions
        .def_readwrite("gpu_pool_size_bytes", &PipelineConfig::gpu_pool_size_bytes)
        .def_readwrite("cuda_device_id", &PipelineConfig::cuda_device_id)
        .def_readwrite("use_cuda_streams", &PipelineConfig::use_cuda_streams)
        .def_readwrite("gpu_require_strict", &PipelineConfig::gpu_require_strict)
        .def_readwrite("result_location", &PipelineConfig::result_location)
        .def_readwrite("shard_row_begin", &PipelineConfig::shard_row_begin)
        .def_readwrite("shard_row_end", &PipelineConfig::shard_row_end)
        .def_readwrite("shard_halo_rows", &PipelineConfig::shard_halo_rows)
        .def_readwrite("scatter_path", &PipelineConfig::scatter_path)
        .def_readwrite("finalize_with_first_ingest", &PipelineConfig::finalize_with_first_ingest)
        .def_readwrite("fill_nodata_radius", &PipelineConfig::fill_nodata_radius)
        .def_readwrite("ground", &PipelineConfig::ground)
        .def_readwrite("terrain", &PipelineConfig::terrain)
        .def_readwrite("trees", &PipelineConfig::trees,
                       "Individual trees: two bands per entry, tree_id and tree_height of the named band, appended behind the terrain "
                       "bands at finalize() (assign a list of TreeBandConfig); Pipeline.trees(i) reads an entry's table")
        .def_readwrite("las_gps_time_origin", &PipelineConfig::las_gps_time_origin)
        .def_readwrite("surface_channels", &PipelineConfig::surface_channels,
                       "Per-point Float32 channels derived at every ingest from a band given with Pipeline.set_surface (assign a "
                       "list of SurfaceChannelConfig): usable wherever a channel is named")
        .def_readwrite("polygon_channels", &PipelineConfig::polygon_channels,
                       "Per-point Float32 channels derived at every ingest from polygons given with Pipeline.set_polygons (assign a "
                       "list of PolygonChannelConfig): the exact per-point test, usable wherever a channel is named")
        .def_readwrite("histograms", &PipelineConfig::histograms,
                       "Per-cell histograms counted at every ingest and the percentile bands finalize() appends behind the "
                       "reductions' bands (assign a list of HistogramConfig)")
        .def_readwrite("extremes", &PipelineConfig::extremes,
                       "Per-cell k lowest / highest distinct values kept at every ingest and the outlier-free Min / Max band "
                       "finalize() appends behind the percentile bands (assign a list of ExtremesConfig)")
        .def_readwrite("cell_stats", &PipelineConfig::cell_stats,
                       "Per-cell integer sums kept at every ingest and the exact Mean / Variance / StdDev bands finalize() appends "
                       "behind the extremes' bands (assign a list of CellStatsConfig)")
        .def_readwrite("zonal", &PipelineConfig::zonal,
                       "Zonal tables: Pipeline.zonal(i) folds the chosen cell_stats planes and histogram cubes by a label band into "
                       "one row per zone (assign a list of ZonalConfig); nothing happens at ingest or in finalize()")
        .def_readwrite("point_zonal", &PipelineConfig::point_zonal,
                       "Point zonal tables: every ingest folds each entry's specs by its per-point label channel into one row per zone "
                       "(assign a list of PointZonalConfig); Pipeline.point_zonal(i) reads the table at any time");

    py::class_<ProgressInfo>(m, "ProgressInfo")
        .def(py::init<>())
        .def_readwrite("collections_processed", &ProgressInfo::collections_processed)
        .def_readwrite("collections_total", &ProgressInfo::collections_total)
        .def_readwrite("points_processed", &ProgressInfo::points_processed)
        .def_readwrite("tiles_active", &ProgressInfo::tiles_active)
        .def_readwrite("elapsed_seconds", &ProgressInfo::elapsed_seconds)
        .def("__repr__", [](const ProgressInfo& p) {
            return "ProgressInfo(points=" + std::to_string(p.points_processed) + ", tiles=" +
                   std::to_string(p.tiles_active) + ", elapsed=" + std::to_string(p.elapsed_seconds) + "s)";
        });

    py::class_<Pipeline>(m, "Pipeline")
        .def_static("create", &Pipeline::create)      // None on failure; reason: pcr.pipeline_create_error()
        .def("validate", [](const Pipeline& p) { raise_if_error(p.validate()); })
        .def("ingest", [](Pipeline& p, const PointCloud& c) { raise_if_error(p.ingest(c)); })
        .def("ingest_async", [](Pipeline& p, const PointCloud& c) { raise_if_error(p.ingest_async(c)); }, py::arg("cloud"),
             "ingest without waiting when the cloud is page-locked or device-resident (keep it alive until synchronize())")
        .def("ingest_file", [](Pipeline& p, const std::string& path, size_t chunk_points) {
            size_t n = 0;
            {
                py::gil_scoped_release release;
                raise_if_error(p.ingest_file(path, chunk_points, &n));
            }
            return n;
        }, py::arg("path"), py::arg("chunk_points") = size_t(4) << 20,
             "stream a PCRP / CSV / LAS file through page-locked double buffers; returns the number of points read")
        .def("set_surface", [](Pipeline& p, const std::string& name, const Grid& grid, int band) {
            raise_if_error(p.set_surface(name, grid, band));
        }, py::arg("name"), py::arg("grid"), py::arg("band") = 0,
             "Gives the surface channel `name` its surface: band `band` of a grid that carries its geometry, copied into the pipeline")
        .def("set_polygons", [](Pipeline& p, const std::string& name, const PolygonSet& polygons, float background, int index_cols,
                                int index_rows) {
            PointInPolygonOptions o;
            o.background = background;
            o.index_cols = index_cols;
            o.index_rows = index_rows;
            raise_if_error(p.set_polygons(name, polygons, o));
        }, py::arg("name"), py::arg("polygons"), py::arg("background") = std::numeric_limits<float>::quiet_NaN(),
             py::arg("index_cols") = 0, py::arg("index_rows") = 0,
             "Gives the polygon channel `name` its polygons (in the grid's CRS): the index is built and kept by the pipeline")
        .def("histogram", [](const Pipeline& p, int i) {
            std::vector<uint32_t> counts;
            raise_if_error(p.histogram_counts(i, &counts));
            int bins = 0, rows = 0, width = 0;
            raise_if_error(p.histogram_shape(i, &bins, &rows, &width));
            py::array_t<uint32_t> out({(py::ssize_t)bins, (py::ssize_t)rows, (py::ssize_t)width});
            if (counts.size() != (size_t)out.size()) throw std::runtime_error("pipeline: histogram: unexpected cube size");
            std::memcpy(out.mutable_data(), counts.data(), counts.size() * sizeof(uint32_t));
            return out;
        }, py::arg("i") = 0,
             "The cube of histogram i as a numpy.uint32 array (bins, height, width): a host copy, valid after any ingest")
        .def("extremes", [](const Pipeline& p, int i) {
            std::vector<float> values;
            raise_if_error(p.extremes_values(i, &values));
            int k = 0, rows = 0, width = 0;
            raise_if_error(p.extremes_shape(i, &k, &rows, &width));
            py::array_t<float> out({(py::ssize_t)k, (py::ssize_t)rows, (py::ssize_t)width});
            if (values.size() != (size_t)out.size()) throw std::runtime_error("pipeline: extremes: unexpected size");
            std::memcpy(out.mutable_data(), values.data(), values.size() * sizeof(float));
            return out;
        }, py::arg("i") = 0,
             "The values extremes entry i keeps as a numpy.float32 array (k, height, width), ascending (Lowest) or descending "
             "(Highest), NaN for an empty slot: a host copy, valid after any ingest")
        .def("cell_stats", [](const Pipeline& p, int i) {
            std::vector<uint32_t> n;
            std::vector<int64_t> s1;
            std::vector<uint64_t> s2;
            raise_if_error(p.cell_stats_state(i, &n, &s1, &s2));
            int rows = 0, width = 0;
            raise_if_error(p.cell_stats_shape(i, &rows, &width));
            py::array_t<uint32_t> an({(py::ssize_t)rows, (py::ssize_t)width});
            py::array_t<int64_t> a1({(py::ssize_t)rows, (py::ssize_t)width});
            py::array_t<uint64_t> a2({(py::ssize_t)rows, (py::ssize_t)width});
            if (n.size() != (size_t)an.size() || s1.size() != n.size() || s2.size() != n.size())
                throw std::runtime_error("pipeline: cell_stats: unexpected size");
            std::memcpy(an.mutable_data(), n.data(), n.size() * sizeof(uint32_t));
            std::memcpy(a1.mutable_data(), s1.data(), s1.size() * sizeof(int64_t));
            std::memcpy(a2.mutable_data(), s2.data(), s2.size() * sizeof(uint64_t));
            return py::make_tuple(an, a1, a2);
        }, py::arg("i") = 0,
             "The state of cell_stats entry i as (N, S1, S2): numpy uint32, int64 and uint64 arrays (height, width) -- the count, "
             "the sum of the steps and the sum of their squares: host copies, valid after any ingest")
        .def("trees", [](const Pipeline& p, int i) {
            TreeTable t;
            raise_if_error(p.trees(i, &t));
            return tree_table_dict(t);
        }, py::arg("i") = 0,
             "The table of trees entry i of the last finalize as a dict of numpy arrays row, col, x, y, height, crown_cells; row k "
             "is the tree with id k + 1")
        .def("set_zones", [](Pipeline& p, const std::string& name, const Grid& grid, int band) {
            raise_if_error(p.set_zones(name, grid, band));
        }, py::arg("name"), py::arg("grid"), py::arg("band") = 0,
             "Gives the external label grid `name` of a ZonalConfig its labels: band `band` of a grid with the pipeline's width and "
             "height, copied into the pipeline")
        .def("set_zones", [](Pipeline& p, const std::string& name, const PolygonSet& polygons, float background) {
            RasterizeOptions o;
            o.background = background;
            raise_if_error(p.set_zones(name, polygons, o));
        }, py::arg("name"), py::arg("polygons"), py::arg("background") = std::numeric_limits<float>::quiet_NaN(),
             "... or burns them from a PolygonSet on the pipeline's grid (pcr.rasterize_polygons' rule): in HBM on the HIP engine")
        .def("polygonize", [](const Pipeline& p, const std::string& band_name) {
            PolygonSet out;
            raise_if_error(p.polygonize(band_name, &out));
            return out;
        }, py::arg("band_name"),
             "The zones of the result's band `band_name` as a PolygonSet on the pipeline's grid (pcr.polygonize's rule), from the "
             "band as the last finalize left it: in HBM on the HIP engine")
        .def("zonal", [](const Pipeline& p, int i) {
            ZonalTable t;
            raise_if_error(p.zonal(i, &t));
            return zone_dict(t.zone, "cells", t.cells, t.stats, t.hists);
        }, py::arg("i") = 0,
             "The table of zonal entry i as a dict of numpy arrays: zone (int32), cells (int64), per cell_stats entry "
             "{channel}_n (uint64), _mean, _var, _std (float32), per histogram {channel}_hist_n (uint64) and {channel}_p{round(q*100)} "
             "(float32); row k is zone k + 1.  Valid after a finalize with no ingest since")
        .def("zonal_histogram", [](const Pipeline& p, int i, int h) {
            ZonalTable t;
            raise_if_error(p.zonal(i, &t, true));
            return zone_histogram("zonal_histogram", t.size(), t.hists, h);
        }, py::arg("i") = 0, py::arg("h") = 0,
             "The (zones, bins) uint64 counts of the h-th histogram chosen by zonal entry i")
        .def("point_zonal", [](const Pipeline& p, int i) {
            PointZonalTable t;
            raise_if_error(p.point_zonal(i, &t));
            return point_zonal_dict(t);
        }, py::arg("i") = 0,
             "The table of point_zonal entry i as a dict of numpy arrays: zone (int32), points (int64), per stats spec {channel}_n "
             "(uint64), _mean, _var, _std (float32), per histogram {channel}_hist_n (uint64) and {channel}_p{round(q*100)} (float32); "
             "row k is zone k + 1.  Valid after any ingest; finalize() is not needed and does not change it")
        .def("point_zonal_histogram", [](const Pipeline& p, int i, int h) {
            PointZonalTable t;
            raise_if_error(p.point_zonal(i, &t, true));
            return zone_histogram("point_zonal_histogram", t.size(), t.hists, h);
        }, py::arg("i") = 0, py::arg("h") = 0, "The (zones, bins) uint64 counts of the h-th histogram of point_zonal entry i")
        .def("finalize", [](Pipeline& p) { raise_if_error(p.finalize()); })
        .def("finalize_async", [](Pipeline& p) { raise_if_error(p.finalize_async()); },
             "Device-resident result: the finalize kernels are only enqueued on the pipeline's stream (complete after synchronize()); "
             "otherwise as finalize()")
        .def("run", [](Pipeline& p, const std::vector<const PointCloud*>& cs) { raise_if_error(p.run(cs)); })
        .def("set_progress_callback", &Pipeline::set_progress_callback)
        .def("result", &Pipeline::result, py::return_value_policy::reference_internal)
        .def("stats", &Pipeline::stats)
        .def("save_state", [](Pipeline& p, const std::string& dir) { raise_if_error(p.save_state(dir)); },
             py::arg("dir") = "")
        .def("load_state", [](Pipeline& p, const std::string& dir) { raise_if_error(p.load_state(dir)); },
             py::arg("dir") = "")
        // extensions for row-block sharded (multi-GPU) runs
        .def("halo_rows", &Pipeline::halo_rows)
        .def("line_reach_rows", [](Pipeline& p, const PointCloud& cloud) {
            int rows = 0;
            raise_if_error(p.line_reach_rows(cloud, &rows));
            return rows;
        })
        .def("state_row_begin", &Pipeline::state_row_begin)
        .def("state_row_count", &Pipeline::state_row_count)
        .def("state_planes", [](const Pipeline& p) {
            py::list out;
            for (const auto& v : p.state_planes())
                out.append(py::make_tuple(reinterpret_cast<uintptr_t>(v.device_ptr), v.plane_kind, v.group));
            return out;
        })
        .def("reduction_groups", &Pipeline::reduction_groups, "Accumulation group of every ReductionSpec (the group of state_planes())")
        .def("plane_reach_rows", [](const Pipeline& p) {
            py::list out;                       // aligned with state_planes(): 0 = the plane's halo rows stay empty (Point glyph)
            for (const auto& v : p.state_planes()) out.append(v.reach_rows);
            return out;
        })
        .def("tile_touched_ptr", [](const Pipeline& p, bool readonly) {
            int tx = 0, ty = 0;
            const void* d = readonly ? p.tile_touched_device_readonly(&tx, &ty) : p.tile_touched_device(&tx, &ty);
            return py::make_tuple(reinterpret_cast<uintptr_t>(d), tx, ty);
        }, py::arg("readonly") = false,
             "(device pointer, tiles_x, tiles_y) of the touched-tile flags; readonly=True promises not to write them (bands a "
             "scatter stored stay valid)")
        .def("merge_touched", [](Pipeline& p, uintptr_t d_union) {
            raise_if_error(p.merge_touched(reinterpret_cast<const void*>(d_union)));
        }, "OR the all-reduced touched flags of every rank (device words) into this pipeline's flags, on its stream")
        .def("result_band_device_ptr", [](const Pipeline& p, int band) { return reinterpret_cast<uintptr_t>(p.result_band_device(band)); },
             "Device address of finished band `band` (own rows x width floats) after finalize(); 0 when there is none")
        .def("synchronize", [](Pipeline& p) { raise_if_error(p.synchronize()); })
        .def("stream_ptr", [](const Pipeline& p) { return reinterpret_cast<uintptr_t>(p.stream_handle()); })
        .def("profile_enable", &Pipeline::profile_enable, py::arg("on"), py::arg("only_kernel") = "")
        .def("profile_read", [](Pipeline& p, bool reset) {
            py::dict d;
            for (const auto& k : p.profile_read(reset))
                d[py::str(k.name)] = py::make_tuple(k.launches, k.total_ms);
            return d;
        }, py::arg("reset") = true)
        .def("last_scatter", [](const Pipeline& p) {
            auto s = p.last_scatter();
            py::dict d;
            d["path"] = s.path == 2 ? "moments" : s.path == 1 ? "binned" : "direct";
            d["lds_tile"] = py::make_tuple(s.lds_tile_w, s.lds_tile_h);
            d["lds_apron"] = s.lds_apron;
            d["num_bins"] = s.num_bins;
            d["points_in"] = s.points_in;
            d["points_valid"] = s.points_valid;
            d["scatter_chunk"] = s.scatter_chunk;
            d["bands_with_scatter"] = s.bands_with_scatter;
            d["deferred_planes"] = s.deferred_planes;
            return d;
        })
        .def("engine", [](const Pipeline& p) { return std::string(p.engine()); },
             "'hip' (the MI355X engine) or 'host' (ExecutionMode.CPU, or a fallback the reference would have taken too)")
        .def("host_threads", &Pipeline::host_threads, "OpenMP threads of the host engine; 0 on the HIP engine")
        .def("spill_dir", &Pipeline::spill_dir, "Out of core: the directory of evicted bands (`.pcrt` tiles, reference layout); '' otherwise")
        .def("out_of_core", &Pipeline::out_of_core,
             "True when the grid's state exceeds gpu_memory_budget and the pipeline sweeps it in row bands of whole reference-tile rows");

    // pcr.distributed: what rank 0 does to the gathered grid -- PipelineConfig.ground, then fill_nodata_radius, then
    // PipelineConfig.terrain -- and the checks of PipelineConfig.ground and .terrain that Pipeline.create makes (the ranks' own
    // configurations carry none of these fields)
    m.def("_finish_gathered", [](const Grid& gathered, const PipelineConfig& whole_cfg) {
        std::unique_ptr<Grid> whole = gathered.to(MemoryLocation::Host);
        if (!whole) throw std::runtime_error("pipeline: failed to copy the gathered grid");
        raise_if_error(detail::finish_gathered_host(whole, whole_cfg));
        return whole;
    }, py::arg("gathered"), py::arg("whole_cfg"));
    m.def("_check_ground", [](const PipelineConfig& whole_cfg) {
        detail::GroundPlan plan;
        raise_if_error(detail::plan_ground(whole_cfg, &plan));
    }, py::arg("whole_cfg"));
    m.def("_check_terrain", [](const PipelineConfig& whole_cfg) {
        detail::GroundPlan ground;
        detail::TerrainPlan plan;
        raise_if_error(detail::plan_ground(whole_cfg, &ground));
        raise_if_error(detail::plan_terrain(whole_cfg, ground, &plan));
    }, py::arg("whole_cfg"));
    m.def("pipeline_create_error", &pipeline_create_error,
          "Why the last Pipeline.create() on this thread returned None");
    m.def("device_count", &cuda_device_count);
    m.def("device_name", &cuda_device_name, py::arg("device_id") = 0);

    // ---- the C++ ShardedPipeline (native RCCL exchange, pcr/engine/sharded_pipeline.h)
    py::class_<ShardedPipeline>(m, "NativeShardedPipeline")
        .def_static("make_id", []() {
            uint8_t id[ShardedPipeline::kIdBytes];
            raise_if_error(ShardedPipeline::make_id(id));
            return py::bytes(reinterpret_cast<const char*>(id), ShardedPipeline::kIdBytes);
        })
        .def_static("row_block", &ShardedPipeline::row_block, py::arg("rank"), py::arg("world"), py::arg("height"),
                    py::arg("align") = 1)
        .def_static("create", [](const PipelineConfig& cfg, const py::bytes& id, int rank, int world, int device, int align) {
            const std::string s = id;
            if (s.size() != (size_t)ShardedPipeline::kIdBytes) throw std::runtime_error("NativeShardedPipeline: the id must be 128 bytes");
            return ShardedPipeline::create(cfg, reinterpret_cast<const uint8_t*>(s.data()), rank, world, device, align);
        }, py::arg("cfg"), py::arg("id"), py::arg("rank"), py::arg("world"), py::arg("device"), py::arg("align") = 1)
        .def_static("create_error", &ShardedPipeline::create_error)
        .def("ingest", [](ShardedPipeline& p, const PointCloud& c) { raise_if_error(p.ingest(c)); })
        .def("exchange", [](ShardedPipeline& p) { raise_if_error(p.exchange()); })
        .def("finalize", [](ShardedPipeline& p) { raise_if_error(p.finalize()); })
        .def("save_state", [](ShardedPipeline& p, const std::string& dir) { raise_if_error(p.save_state(dir)); }, py::arg("dir") = "")
        .def("load_state", [](ShardedPipeline& p, const std::string& dir) { raise_if_error(p.load_state(dir)); }, py::arg("dir") = "")
        .def("ingest_unrouted", [](ShardedPipeline& p, const PointCloud& c) {
            size_t got = 0;
            raise_if_error(p.ingest_unrouted(c, &got));
            return got;
        }, "An arbitrary shard of the cloud: partitioned by owner on the device, exchanged (pcr_hip_comm_alltoallv), ingested; -> points received")
        .def("gather", [](ShardedPipeline& p, int dst_rank) {
            std::unique_ptr<Grid> g;
            raise_if_error(p.gather(dst_rank, &g));
            return g;
        }, py::arg("dst_rank") = 0, "Collective, after finalize(): the whole grid as one host Grid on dst_rank, None elsewhere")
        .def("result", &ShardedPipeline::result, py::return_value_policy::reference_internal)
        .def("pipeline", &ShardedPipeline::pipeline, py::return_value_policy::reference_internal)
        .def("row_begin", &ShardedPipeline::row_begin)
        .def("row_end", &ShardedPipeline::row_end)
        .def("halo_rows", &ShardedPipeline::halo_rows)
        .def("tiles_local", &ShardedPipeline::tiles_local)
        .def("bytes_sent", &ShardedPipeline::bytes_sent);
}
