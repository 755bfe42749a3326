// bind_io.cpp -- the reference's I/O layer at the same Python names (python/bindings.cpp:500-640):
// PCRP / CSV point clouds, GeoTIFF output of finalized grids, `.pcrt` tile-state checkpoints.
// LAS files are read (read_point_cloud, read_las, PointCloudReader; not in the reference); writing LAS, and LAZ either way,
// raise NotImplemented as upstream.
#include "common.h"

#include "pcr/core/fill_nodata.h"
#include "pcr/core/grid.h"
#include "pcr/core/grid_config.h"
#include "pcr/core/ground_filter.h"
#include "pcr/core/point_cloud.h"
#include "pcr/io/grid_io.h"
#include "pcr/io/point_cloud_io.h"
#include "pcr/io/tile_state_io.h"
#include "../../host/src/ground_filter.h"

#include <vector>

using namespace pcr;

void bind_io(py::module_& m) {
    // `.pcrt` tile-state files (the reference's checkpoint format) -- implemented, unlike the rest of I/O
    m.def("write_tile_state", [](const std::string& path, int tile_row, int tile_col,
                                 py::array_t<float, py::array::c_style | py::array::forcecast> state,
                                 ReductionType type) {
        auto b = state.request();
        if (b.ndim != 3) throw std::runtime_error("write_tile_state: state must be [state_floats, rows, cols]");
        TileIndex t;
        t.row = tile_row;
        t.col = tile_col;
        raise_if_error(write_tile_state(path, t, (int)b.shape[2], (int)b.shape[1], (int)b.shape[0], type,
                                        static_cast<const float*>(b.ptr)));
    }, py::arg("path"), py::arg("tile_row"), py::arg("tile_col"), py::arg("state"), py::arg("type"));
    m.def("read_tile_state", [](const std::string& path) {
        TileIndex t;
        int cols = 0, rows = 0, k = 0;
        ReductionType type;
        raise_if_error(read_tile_state_header(path, t, cols, rows, k, type));
        py::array_t<float> out({k, rows, cols});
        raise_if_error(read_tile_state(path, t, cols, rows, k, type, out.mutable_data()));
        return py::make_tuple(t.row, t.col, out, type);
    }, py::arg("path"));
    m.def("tile_state_filename", [](const std::string& dir, int tile_row, int tile_col) {
        TileIndex t;
        t.row = tile_row;
        t.col = tile_col;
        return tile_state_filename(dir, t);
    });

    py::enum_<PointCloudFormat>(m, "PointCloudFormat")
        .value("PCR_Binary", PointCloudFormat::PCR_Binary).value("CSV", PointCloudFormat::CSV)
        .value("LAS", PointCloudFormat::LAS).value("LAZ", PointCloudFormat::LAZ)
        .value("Auto", PointCloudFormat::Auto).export_values();

    py::class_<GeoTiffOptions>(m, "GeoTiffOptions")
        .def(py::init<>())
        .def_readwrite("cloud_optimized", &GeoTiffOptions::cloud_optimized)
        .def_readwrite("compress", &GeoTiffOptions::compress)
        .def_readwrite("compress_level", &GeoTiffOptions::compress_level)
        .def_readwrite("tile_width", &GeoTiffOptions::tile_width)
        .def_readwrite("tile_height", &GeoTiffOptions::tile_height)
        .def_readwrite("bigtiff", &GeoTiffOptions::bigtiff)
        .def_readwrite("overview_resampling", &GeoTiffOptions::overview_resampling)
        .def_readwrite("overviews", &GeoTiffOptions::overviews);

    py::class_<PointCloudInfo>(m, "PointCloudInfo")
        .def(py::init<>())
        .def_readwrite("num_points", &PointCloudInfo::num_points)
        .def_readwrite("channels", &PointCloudInfo::channels)
        .def_readwrite("crs", &PointCloudInfo::crs)
        .def_readwrite("bounds", &PointCloudInfo::bounds);

    py::class_<PointCloudReader>(m, "PointCloudReader")
        .def_static("open", [](const std::string& path, PointCloudFormat format, py::object channels, double gps_time_origin) {
            LasOptions las;                                     // (only a LAS file looks at it)
            if (!channels.is_none()) las.channels = channels.cast<std::vector<std::string>>();
            las.gps_time_origin = gps_time_origin;
            Status s;
            auto r = PointCloudReader::open(path, format, &las, &s);
            if (!r) throw std::runtime_error("Failed to open point cloud: " + path + (s.message.empty() ? "" : ": " + s.message));
            return r;
        }, py::arg("path"), py::arg("format") = PointCloudFormat::Auto, py::arg("channels") = py::none(),
           py::arg("gps_time_origin") = 0.0)
        .def("format", &PointCloudReader::format)
        .def("info", &PointCloudReader::info, py::return_value_policy::reference_internal)
        .def("read_chunk", &PointCloudReader::read_chunk, py::arg("cloud"), py::arg("max_points"))
        .def("rewind", [](PointCloudReader& r) { raise_if_error(r.rewind()); })
        .def("eof", &PointCloudReader::eof);

    // extension (the reference does not bind it): incremental assembly from reference tiles
    py::class_<TiledGeoTiffWriter>(m, "TiledGeoTiffWriter")
        .def_static("open", [](const std::string& path, const GridConfig& config, const std::vector<std::string>& band_names,
                               const GeoTiffOptions& options) {
            auto w = TiledGeoTiffWriter::open(path, config, band_names, options);
            if (!w) throw std::runtime_error("TiledGeoTiffWriter.open: failed to create " + path);
            return w;
        }, py::arg("path"), py::arg("config"), py::arg("band_names"), py::arg("options") = GeoTiffOptions())
        .def("write_tile", [](TiledGeoTiffWriter& w, int tile_row, int tile_col,
                              py::array_t<float, py::array::c_style | py::array::forcecast> data) {
            auto b = data.request();
            if (b.ndim != 3) throw std::runtime_error("write_tile: data must be [bands, rows, cols]");
            TileIndex t;
            t.row = tile_row;
            t.col = tile_col;
            raise_if_error(w.write_tile(t, static_cast<const float*>(b.ptr), (int)b.shape[0]));
        }, py::arg("tile_row"), py::arg("tile_col"), py::arg("data"))
        .def("close", [](TiledGeoTiffWriter& w) { raise_if_error(w.close()); });

    m.def("write_geotiff", [](const std::string& path, const Grid& grid, const GridConfig& config, const GeoTiffOptions& options,
                              py::object overviews) {
        std::vector<const Grid*> levels;                    // None: built by the writer when options.overviews != 0
        if (!overviews.is_none()) levels = overviews.cast<std::vector<const Grid*>>();
        raise_if_error(write_geotiff(path, grid, config, options, levels));
    }, py::arg("path"), py::arg("grid"), py::arg("config"), py::arg("options") = GeoTiffOptions(),
       py::arg("overviews") = py::none());
    // extension: the overview levels of a grid, made where it lives (a Device grid: in HBM)
    m.def("build_overviews", [](const Grid& grid, int levels, const std::string& resampling) {
        Status s;
        auto out = build_overviews(grid, levels, resampling, &s, nullptr);
        raise_if_error(s);
        return out;
    }, py::arg("grid"), py::arg("levels") = -1, py::arg("resampling") = "average");
    // extension: the NaN cells of a grid's bands filled from their valid neighbours, where the grid lives (a Device grid: in HBM)
    m.def("fill_nodata", [](const Grid& grid, int radius, py::object bands) {
        std::vector<int> list;                              // None: every band
        if (!bands.is_none()) list = bands.cast<std::vector<int>>();
        Status s;
        auto out = fill_nodata(grid, radius, list, &s, nullptr);
        raise_if_error(s);
        return out;
    }, py::arg("grid"), py::arg("radius"), py::arg("bands") = py::none());
    // extension: the ground filter (a DTM band, and height above ground) of a grid's band, where the grid lives
    m.def("ground_filter", [](const Grid& grid, int band, py::object spec, double cell_size, py::object top_band) {
        Status s;
        auto out = ground_filter(grid, band, spec.is_none() ? GroundFilterSpec() : spec.cast<GroundFilterSpec>(), cell_size,
                                 top_band.is_none() ? -1 : top_band.cast<int>(), &s, nullptr);
        raise_if_error(s);
        return out;
    }, py::arg("grid"), py::arg("band") = 0, py::arg("spec") = py::none(), py::arg("cell_size") = 1.0, py::arg("top_band") = py::none());
    m.def("ground_filter_levels", [](const GroundFilterSpec& spec, double cell_size) {
        std::vector<int> radii;
        std::vector<float> thresholds;
        raise_if_error(ground_filter_levels(spec, cell_size, &radii, &thresholds));
        return py::make_tuple(radii, thresholds);
    }, py::arg("spec"), py::arg("cell_size") = 1.0);
    // (tests, tools) the host loop on an array with explicit levels, which the kernels are compared with level by level
    m.def("_ground_filter_host", [](py::array_t<float, py::array::c_style | py::array::forcecast> src, const std::vector<int>& radii,
                                    const std::vector<float>& thresholds) {
        if (src.ndim() != 2 || src.shape(0) < 1 || src.shape(1) < 1) throw std::invalid_argument("ground_filter: a 2-D array is needed");
        if (radii.empty() || radii.size() != thresholds.size() || radii.size() > 64)
            throw std::invalid_argument("ground_filter: levels must be between 1 and 64");
        for (size_t k = 0; k < radii.size(); ++k)
            if (radii[k] < 1 || radii[k] > 64 || (k && radii[k] <= radii[k - 1]) || !(thresholds[k] >= 0.0f) || !std::isfinite(thresholds[k]))
                throw std::invalid_argument("ground_filter: invalid level");
        const int h = (int)src.shape(0), w = (int)src.shape(1);
        py::array_t<float> out({h, w});
        detail::ground_filter_host(src.data(), out.mutable_data(), w, h, w, w, (int)radii.size(), radii.data(), thresholds.data());
        return out;
    }, py::arg("src"), py::arg("radii"), py::arg("thresholds"));
    m.def("read_geotiff_overviews", [](const std::string& path) {
        std::vector<std::pair<int, int>> sizes;
        raise_if_error(read_geotiff_overviews(path, sizes));
        return sizes;
    }, py::arg("path"));
    m.def("read_geotiff_info", [](const std::string& path) {
        int w = 0, h = 0, nb = 0;
        CRS crs;
        BBox bounds;
        raise_if_error(read_geotiff_info(path, w, h, nb, crs, bounds));
        return py::make_tuple(w, h, nb, crs, bounds);
    }, py::arg("path"));
    m.def("read_geotiff_band", [](const std::string& path, int band_index, int level) {
        int w = 0, h = 0, nb = 0;
        CRS crs;
        BBox bounds;
        raise_if_error(read_geotiff_info(path, w, h, nb, crs, bounds));
        if (level != 0) {
            std::vector<std::pair<int, int>> sizes;
            raise_if_error(read_geotiff_overviews(path, sizes));
            if (level < 0 || level > (int)sizes.size()) throw std::runtime_error("read_geotiff_band: overview level out of range");
            w = sizes[(size_t)level - 1].first;
            h = sizes[(size_t)level - 1].second;
        }
        py::array_t<float> out({h, w});
        raise_if_error(read_geotiff_band_level(path, level, band_index, out.mutable_data(), w, h));
        return out;
    }, py::arg("path"), py::arg("band_index") = 0, py::arg("level") = 0);
    m.def("read_geotiff_band_names", [](const std::string& path) {
        std::vector<std::string> names;
        raise_if_error(read_geotiff_band_names(path, names));
        return names;
    }, py::arg("path"));

    m.def("read_point_cloud", [](const std::string& path, PointCloudFormat format, MemoryLocation location) {
        auto c = read_point_cloud(path, format, location);
        if (!c) throw std::runtime_error("Failed to read point cloud: " + path);
        return c;
    }, py::arg("path"), py::arg("format") = PointCloudFormat::Auto, py::arg("location") = MemoryLocation::Host);
    // extension: a LAS file with a choice of channels (None: all the point format has) and a GPS time origin
    m.def("read_las", [](const std::string& path, py::object channels, double gps_time_origin, MemoryLocation location) {
        LasOptions las;
        if (!channels.is_none()) las.channels = channels.cast<std::vector<std::string>>();
        las.gps_time_origin = gps_time_origin;
        Status s;
        auto c = read_las(path, las, location, &s);
        if (!c) throw std::runtime_error(s.message.empty() ? "Failed to read point cloud: " + path : s.message);
        return c;
    }, py::arg("path"), py::arg("channels") = py::none(), py::arg("gps_time_origin") = 0.0,
       py::arg("location") = MemoryLocation::Host);
    m.def("write_point_cloud", [](const std::string& path, const PointCloud& cloud, PointCloudFormat format) {
        raise_if_error(write_point_cloud(path, cloud, format));
    }, py::arg("path"), py::arg("cloud"), py::arg("format") = PointCloudFormat::PCR_Binary);
    m.def("read_point_cloud_info", [](const std::string& path, PointCloudFormat format) {
        PointCloudInfo info;
        raise_if_error(read_point_cloud_info(path, info, format));
        return info;
    }, py::arg("path"), py::arg("format") = PointCloudFormat::Auto);
}
