// bind_core.cpp -- enums, BBox/CRS/..., GridConfig, Grid, PointCloud.
#include "common.h"

#include "pcr/core/grid.h"
#include "pcr/core/grid_config.h"
#include "pcr/core/ground_filter.h"
#include "pcr/core/point_cloud.h"
#include "pcr/core/polygons.h"
#include "pcr/core/reproject.h"
#include "pcr/core/sample_grid.h"
#include "pcr/core/terrain.h"
#include "pcr/core/trees.h"
#include "pcr/engine/pipeline.h"
#include "pcr_hip.h"
#include "../../host/src/pipeline_common.h"
#include "../../host/src/terrain.h"
#include "../../host/src/trees.h"

#include <cstring>

#include <omp.h>

using namespace pcr;

namespace {

std::string num(double v) { return std::to_string(v); }

template <typename T>
py::array_t<T> host_view(T* data, size_t n, py::handle owner, const char* what) {
    if (!data) throw std::runtime_error(std::string(what) + ": no data");
    return py::array_t<T>({static_cast<py::ssize_t>(n)}, {static_cast<py::ssize_t>(sizeof(T))}, data, owner);
}

void require_host(MemoryLocation loc, const char* what) {
    if (loc == MemoryLocation::Device)
        throw std::runtime_error(std::string(what) + ": data lives in Device memory; call to_host() first");
}

template <typename T>
void copy_in(T* dst, const py::array_t<T, py::array::c_style | py::array::forcecast>& arr, size_t limit,
             const char* too_big) {
    auto buf = arr.request();
    if (buf.ndim != 1) throw std::runtime_error("expected a 1-D array");
    if (static_cast<size_t>(buf.shape[0]) > limit) throw std::runtime_error(too_big);
    std::memcpy(dst, buf.ptr, static_cast<size_t>(buf.shape[0]) * sizeof(T));
}

}  // namespace

void bind_core(py::module_& m) {
    py::enum_<DataType>(m, "DataType")
        .value("Float32", DataType::Float32).value("Float64", DataType::Float64)
        .value("Int32", DataType::Int32).value("UInt32", DataType::UInt32)
        .value("Int16", DataType::Int16).value("UInt16", DataType::UInt16)
        .value("UInt8", DataType::UInt8).export_values();

    py::enum_<ReductionType>(m, "ReductionType")
        .value("Sum", ReductionType::Sum).value("Max", ReductionType::Max).value("Min", ReductionType::Min)
        .value("Average", ReductionType::Average).value("WeightedAverage", ReductionType::WeightedAverage)
        .value("Count", ReductionType::Count).value("Median", ReductionType::Median)
        .value("Percentile", ReductionType::Percentile).value("MostRecent", ReductionType::MostRecent)
        .value("PriorityMerge", ReductionType::PriorityMerge).value("Custom", ReductionType::Custom)
        .export_values();

    py::enum_<MemoryLocation>(m, "MemoryLocation")
        .value("Host", MemoryLocation::Host).value("HostPinned", MemoryLocation::HostPinned)
        .value("Device", MemoryLocation::Device).export_values();

    py::enum_<StatusCode>(m, "StatusCode")
        .value("Ok", StatusCode::Ok).value("InvalidArgument", StatusCode::InvalidArgument)
        .value("OutOfMemory", StatusCode::OutOfMemory).value("CudaError", StatusCode::CudaError)
        .value("IoError", StatusCode::IoError).value("CrsError", StatusCode::CrsError)
        .value("NotImplemented", StatusCode::NotImplemented).value("OutOfRange", StatusCode::OutOfRange).export_values();

    py::class_<BBox>(m, "BBox")
        .def(py::init<>())
        .def(py::init([](double x0, double y0, double x1, double y1) {
                 BBox b; b.min_x = x0; b.min_y = y0; b.max_x = x1; b.max_y = y1; return b; }),
             py::arg("min_x"), py::arg("min_y"), py::arg("max_x"), py::arg("max_y"))
        .def_readwrite("min_x", &BBox::min_x).def_readwrite("min_y", &BBox::min_y)
        .def_readwrite("max_x", &BBox::max_x).def_readwrite("max_y", &BBox::max_y)
        .def("expand", py::overload_cast<double, double>(&BBox::expand))
        .def("expand", py::overload_cast<const BBox&>(&BBox::expand))
        .def("contains", &BBox::contains)
        .def("width", &BBox::width).def("height", &BBox::height).def("valid", &BBox::valid)
        .def("__repr__", [](const BBox& b) {
            return "BBox(min_x=" + num(b.min_x) + ", min_y=" + num(b.min_y) +
                   ", max_x=" + num(b.max_x) + ", max_y=" + num(b.max_y) + ")";
        });

    py::class_<CRS>(m, "CRS")
        .def(py::init<>())
        .def_readwrite("wkt", &CRS::wkt).def_readwrite("epsg", &CRS::epsg)
        .def("is_projected", &CRS::is_projected).def("is_geographic", &CRS::is_geographic)
        .def("is_valid", &CRS::is_valid)
        .def_static("from_epsg", &CRS::from_epsg).def_static("from_wkt", &CRS::from_wkt)
        .def("equivalent_to", &CRS::equivalent_to)
        .def("__repr__", [](const CRS& c) {
            return c.epsg ? "CRS(epsg=" + std::to_string(c.epsg) + ")" : "CRS(wkt='" + c.wkt.substr(0, 50) + "...')";
        });

    py::class_<NoDataPolicy>(m, "NoDataPolicy")
        .def(py::init<>())
        .def_readwrite("value", &NoDataPolicy::value).def_readwrite("use_nan", &NoDataPolicy::use_nan)
        .def("sentinel", &NoDataPolicy::sentinel);

    py::class_<TileIndex>(m, "TileIndex")
        .def(py::init<>())
        .def(py::init([](int row, int col) { TileIndex t; t.row = row; t.col = col; return t; }))
        .def_readwrite("row", &TileIndex::row).def_readwrite("col", &TileIndex::col)
        .def("__eq__", &TileIndex::operator==).def("__lt__", &TileIndex::operator<)
        .def("__repr__", [](const TileIndex& t) {
            return "TileIndex(row=" + std::to_string(t.row) + ", col=" + std::to_string(t.col) + ")";
        });

    py::class_<Status>(m, "Status")
        .def(py::init<>())
        .def_readwrite("code", &Status::code).def_readwrite("message", &Status::message)
        .def("ok", &Status::ok)
        .def_static("success", &Status::success).def_static("error", &Status::error)
        .def("__bool__", &Status::ok)
        .def("__repr__", [](const Status& s) -> std::string {
            if (s.ok()) return "Status(Ok)";
            return "Status(code=" + std::to_string(static_cast<int>(s.code)) + ", message='" + s.message + "')";
        });

    py::class_<ChannelDesc>(m, "ChannelDesc")
        .def(py::init<>())
        .def_readwrite("name", &ChannelDesc::name).def_readwrite("dtype", &ChannelDesc::dtype)
        .def_readwrite("offset", &ChannelDesc::offset);

    py::class_<BandDesc>(m, "BandDesc")
        .def(py::init<>())
        .def_readwrite("name", &BandDesc::name).def_readwrite("dtype", &BandDesc::dtype)
        .def_readwrite("is_state", &BandDesc::is_state);

    // extension: the level schedule of the ground filter (pcr.ground_filter, PipelineConfig.ground)
    py::class_<GroundFilterSpec>(m, "GroundFilterSpec")
        .def(py::init<>())
        .def_readwrite("max_radius_cells", &GroundFilterSpec::max_radius_cells)
        .def_readwrite("exponential", &GroundFilterSpec::exponential)
        .def_readwrite("slope", &GroundFilterSpec::slope)
        .def_readwrite("initial_distance", &GroundFilterSpec::initial_distance)
        .def_readwrite("max_distance", &GroundFilterSpec::max_distance);

    // extension: the terrain bands (pcr.terrain, PipelineConfig.terrain)
    py::enum_<TerrainProduct>(m, "TerrainProduct")
        .value("SlopeDegrees", TerrainProduct::SlopeDegrees).value("SlopePercent", TerrainProduct::SlopePercent)
        .value("Aspect", TerrainProduct::Aspect).value("Hillshade", TerrainProduct::Hillshade)
        .value("TRI", TerrainProduct::TRI).value("TPI", TerrainProduct::TPI).value("Roughness", TerrainProduct::Roughness);
    py::class_<TerrainSpec>(m, "TerrainSpec")
        .def(py::init<>())
        .def_readwrite("z_factor", &TerrainSpec::z_factor)
        .def_readwrite("compute_edges", &TerrainSpec::compute_edges)
        .def_readwrite("azimuth", &TerrainSpec::azimuth)
        .def_readwrite("altitude", &TerrainSpec::altitude);
    // extension: individual trees (pcr.segment_trees, PipelineConfig.trees)
    py::class_<TreeSpec>(m, "TreeSpec", "Tree tops by a variable-window local-maximum filter and crown labels by seeded descent")
        .def(py::init<>())
        .def(py::init<const TreeSpec&>())
        .def_readwrite("min_height", &TreeSpec::min_height)
        .def_readwrite("window_base", &TreeSpec::window_base)
        .def_readwrite("window_slope", &TreeSpec::window_slope)
        .def_readwrite("max_radius_cells", &TreeSpec::max_radius_cells)
        .def_readwrite("min_crown_height", &TreeSpec::min_crown_height)
        .def_readwrite("crown_ratio", &TreeSpec::crown_ratio)
        .def_readwrite("max_crown_radius", &TreeSpec::max_crown_radius);
    m.def("terrain_light", [](double azimuth, double altitude) {
        const TerrainLight l = terrain_light(azimuth, altitude);
        return py::make_tuple(l.sin_alt, l.ls, l.lc);
    }, py::arg("azimuth") = 315.0, py::arg("altitude") = 45.0,
       "(sin_alt, cos_alt * sin_az, cos_alt * cos_az): the binary64 hillshade constants every engine uses");

    py::class_<GridConfig>(m, "GridConfig")
        .def(py::init<>())
        .def_readwrite("bounds", &GridConfig::bounds).def_readwrite("crs", &GridConfig::crs)
        .def_readwrite("cell_size_x", &GridConfig::cell_size_x).def_readwrite("cell_size_y", &GridConfig::cell_size_y)
        .def_readwrite("width", &GridConfig::width).def_readwrite("height", &GridConfig::height)
        .def_readwrite("nodata", &GridConfig::nodata)
        .def_readwrite("tile_width", &GridConfig::tile_width).def_readwrite("tile_height", &GridConfig::tile_height)
        .def_readwrite("tiles_x", &GridConfig::tiles_x).def_readwrite("tiles_y", &GridConfig::tiles_y)
        .def("compute_dimensions", &GridConfig::compute_dimensions)
        .def("world_to_cell", [](const GridConfig& g, double wx, double wy) {
            int col = 0, row = 0;
            bool ok = g.world_to_cell(wx, wy, col, row);
            return py::make_tuple(col, row, ok);
        })
        .def("cell_to_world", [](const GridConfig& g, int col, int row) {
            double wx = 0, wy = 0;
            g.cell_to_world(col, row, wx, wy);
            return py::make_tuple(wx, wy);
        })
        .def("cell_to_tile", &GridConfig::cell_to_tile)
        .def("tile_bounds", &GridConfig::tile_bounds)
        .def("tile_cell_range", [](const GridConfig& g, TileIndex t) {
            int c0 = 0, r0 = 0, nc = 0, nr = 0;
            g.tile_cell_range(t, c0, r0, nc, nr);
            return py::make_tuple(c0, r0, nc, nr);
        })
        .def("total_tiles", &GridConfig::total_tiles).def("total_cells", &GridConfig::total_cells)
        .def("gdal_geotransform", [](const GridConfig& g) {       // C++-only in the reference; bound for the known-answer tests
            double gt[6];
            g.gdal_geotransform(gt);
            return py::make_tuple(gt[0], gt[1], gt[2], gt[3], gt[4], gt[5]);
        })
        .def("validate", [](const GridConfig& g) { raise_if_error(g.validate()); })
        .def("__repr__", [](const GridConfig& g) {
            return "GridConfig(width=" + std::to_string(g.width) + ", height=" + std::to_string(g.height) +
                   ", tiles=" + std::to_string(g.tiles_x) + "x" + std::to_string(g.tiles_y) + ")";
        });

    py::class_<Grid>(m, "Grid")
        .def_static("create", &Grid::create, py::arg("cols"), py::arg("rows"), py::arg("bands"),
                    py::arg("loc") = MemoryLocation::Host)
        .def_static("create_for_tile", &Grid::create_for_tile, py::arg("config"), py::arg("tile"),
                    py::arg("bands"), py::arg("loc") = MemoryLocation::Host)
        .def("num_bands", &Grid::num_bands).def("band_desc", &Grid::band_desc)
        .def("band_index", &Grid::band_index)
        .def("cols", &Grid::cols).def("rows", &Grid::rows).def("cell_count", &Grid::cell_count)
        .def("location", &Grid::location)
        .def("fill", [](Grid& g, float v) { raise_if_error(g.fill(v)); })
        .def("fill_band", [](Grid& g, int i, float v) { raise_if_error(g.fill_band(i, v)); })
        .def("band_array", [](Grid& g, int i) {
            float* p = g.band_f32(i);
            if (!p) throw std::runtime_error("Invalid band index or data type");
            require_host(g.location(), "band_array");
            return py::array_t<float>({g.rows(), g.cols()},
                                      {static_cast<py::ssize_t>(g.cols() * sizeof(float)),
                                       static_cast<py::ssize_t>(sizeof(float))},
                                      p, py::cast(&g));
        })
        .def("set_band_array", [](Grid& g, int i, py::array_t<float, py::array::c_style | py::array::forcecast> a) {
            float* p = g.band_f32(i);
            if (!p) throw std::runtime_error("Invalid band index or data type");
            require_host(g.location(), "set_band_array");
            auto buf = a.request();
            if (buf.ndim != 2 || buf.shape[0] != g.rows() || buf.shape[1] != g.cols())
                throw std::runtime_error("Array shape mismatch");
            std::memcpy(p, buf.ptr, static_cast<size_t>(g.cell_count()) * sizeof(float));
        })
        // extensions: device-resident results
        .def("band_device_ptr", [](Grid& g, int i) {
            if (g.location() != MemoryLocation::Device) throw std::runtime_error("band_device_ptr: grid is not on Device");
            float* p = g.band_f32(i);
            if (!p) throw std::runtime_error("Invalid band index or data type");
            return reinterpret_cast<uintptr_t>(p);
        })
        .def("to_host", [](const Grid& g) {
            auto h = g.to(MemoryLocation::Host);
            if (!h) throw std::runtime_error("Failed to copy grid to Host memory");
            return h;
        })
        .def("to", [](const Grid& g, MemoryLocation loc) {
            auto d = g.to(loc);
            if (!d) throw std::runtime_error("Failed to copy the grid (HIP out of memory or no usable GPU)");
            return d;
        }, py::arg("location"), "A copy of the grid in `location` (MemoryLocation.Device: in GPU memory)")
        // extension: where the cells lie in the world (pcr.sample_grid, Pipeline.set_surface)
        .def("set_geometry", [](Grid& g, const GridConfig& gc) { raise_if_error(g.set_geometry(gc)); }, py::arg("geometry"),
             "Tags the grid with the GridConfig its cells are laid over (width and height must be cols() and rows())")
        .def("geometry", [](const Grid& g) -> py::object {
            const GridConfig* gc = g.geometry();
            return gc ? py::cast(*gc) : py::none();
        }, "The GridConfig the grid was tagged with (a pipeline tags result() of a whole grid), or None")
        .def("__repr__", [](const Grid& g) {
            return "Grid(cols=" + std::to_string(g.cols()) + ", rows=" + std::to_string(g.rows()) +
                   ", bands=" + std::to_string(g.num_bands()) + ")";
        });

    py::class_<PointCloud>(m, "PointCloud")
        .def_static("create", &PointCloud::create, py::arg("capacity"), py::arg("loc") = MemoryLocation::Host)
        .def("add_channel", [](PointCloud& pc, const std::string& name, DataType dt) {
            raise_if_error(pc.add_channel(name, dt));
        }, py::arg("name"), py::arg("dtype") = DataType::Float32)
        .def("has_channel", &PointCloud::has_channel)
        .def("channel", &PointCloud::channel, py::return_value_policy::reference_internal)
        .def("channel_names", &PointCloud::channel_names)
        .def("count", &PointCloud::count).def("capacity", &PointCloud::capacity)
        .def("location", &PointCloud::location)
        .def("crs", &PointCloud::crs).def("set_crs", &PointCloud::set_crs)
        .def("resize", [](PointCloud& pc, size_t n) { raise_if_error(pc.resize(n)); })
        .def("x_array", [](PointCloud& pc) {
            require_host(pc.location(), "x_array");
            return host_view<double>(pc.x(), pc.count(), py::cast(&pc), "x_array");
        })
        .def("y_array", [](PointCloud& pc) {
            require_host(pc.location(), "y_array");
            return host_view<double>(pc.y(), pc.count(), py::cast(&pc), "y_array");
        })
        .def("channel_array_f32", [](PointCloud& pc, const std::string& name) {
            float* p = pc.channel_f32(name);
            if (!p) throw std::runtime_error("Channel not found or wrong type: " + name);
            require_host(pc.location(), "channel_array_f32");
            return host_view<float>(p, pc.count(), py::cast(&pc), "channel_array_f32");
        })
        // set_x_array also sets the point count (len(arr)); set_y_array only copies -- reference behaviour
        .def("set_x_array", [](PointCloud& pc, py::array_t<double, py::array::c_style | py::array::forcecast> a) {
            require_host(pc.location(), "set_x_array");
            copy_in<double>(pc.x(), a, pc.capacity(), "Array too large for capacity");
            raise_if_error(pc.resize(static_cast<size_t>(a.request().shape[0])));
        })
        .def("set_y_array", [](PointCloud& pc, py::array_t<double, py::array::c_style | py::array::forcecast> a) {
            require_host(pc.location(), "set_y_array");
            copy_in<double>(pc.y(), a, pc.capacity(), "Array too large for capacity");
        })
        .def("set_channel_array_f32", [](PointCloud& pc, const std::string& name,
                                         py::array_t<float, py::array::c_style | py::array::forcecast> a) {
            float* p = pc.channel_f32(name);
            if (!p) throw std::runtime_error("Channel not found or wrong type: " + name);
            require_host(pc.location(), "set_channel_array_f32");
            copy_in<float>(p, a, pc.count(), "Array size exceeds point count");
        })
        // extension: any channel as a zero-copy array of its own dtype (files carry f64 / i32 / u32 channels too)
        .def("channel_array", [](PointCloud& pc, const std::string& name) -> py::object {
            const ChannelDesc* d = pc.channel(name);
            void* p = pc.channel_data(name);
            if (!d || !p) throw std::runtime_error("Channel not found: " + name);
            require_host(pc.location(), "channel_array");
            py::object owner = py::cast(&pc);
            switch (d->dtype) {
                case DataType::Float32: return host_view<float>(static_cast<float*>(p), pc.count(), owner, "channel_array");
                case DataType::Float64: return host_view<double>(static_cast<double*>(p), pc.count(), owner, "channel_array");
                case DataType::Int32: return host_view<int32_t>(static_cast<int32_t*>(p), pc.count(), owner, "channel_array");
                case DataType::UInt32: return host_view<uint32_t>(static_cast<uint32_t*>(p), pc.count(), owner, "channel_array");
                case DataType::Int16: return host_view<int16_t>(static_cast<int16_t*>(p), pc.count(), owner, "channel_array");
                case DataType::UInt16: return host_view<uint16_t>(static_cast<uint16_t*>(p), pc.count(), owner, "channel_array");
                default: return host_view<uint8_t>(static_cast<uint8_t*>(p), pc.count(), owner, "channel_array");
            }
        })
        .def("to_device", [](const PointCloud& pc) {
            auto d = pc.to(MemoryLocation::Device);
            if (!d) throw std::runtime_error("Failed to transfer point cloud to Device memory "
                                             "(HIP out of memory or no usable GPU)");
            return d;
        }, "Copy the cloud (coordinates and every channel) into GPU memory")
        .def("to_host", [](const PointCloud& pc) {
            auto h = pc.to(MemoryLocation::Host);
            if (!h) throw std::runtime_error("Failed to transfer point cloud to Host memory");
            return h;
        }, "Copy the cloud into Host memory")
        // extension: raw device addresses for zero-copy interop (torch / __cuda_array_interface__)
        .def("device_ptrs", [](PointCloud& pc) {
            py::dict d;
            d["x"] = reinterpret_cast<uintptr_t>(pc.x());
            d["y"] = reinterpret_cast<uintptr_t>(pc.y());
            for (const auto& n : pc.channel_names()) d[py::str(n)] = reinterpret_cast<uintptr_t>(pc.channel_data(n));
            return d;
        })
        .def("__repr__", [](const PointCloud& pc) {
            return "PointCloud(count=" + std::to_string(pc.count()) + ", capacity=" + std::to_string(pc.capacity()) +
                   ", channels=" + std::to_string(pc.channel_names().size()) + ")";
        });

    // ---- reprojection (pcr/core/reproject.h); pcr.transform_xy in pcr/__init__.py picks the host or the device form
    m.def("crs_epsg", &crs_epsg, py::arg("crs"),
          "EPSG code of a CRS: CRS.epsg, else the top-level EPSG authority of its WKT; 0 when unidentified");
    m.def("_transform_xy_host", [](const CRS& src, const CRS& dst,
                                   py::array_t<double, py::array::c_style | py::array::forcecast> x,
                                   py::array_t<double, py::array::c_style | py::array::forcecast> y) {
        auto bx = x.request(), by = y.request();
        if (bx.ndim != 1 || by.ndim != 1 || bx.shape[0] != by.shape[0])
            throw std::runtime_error("transform_xy: x and y must be 1-D arrays of the same length");
        const size_t n = static_cast<size_t>(bx.shape[0]);
        py::array_t<double> ox(static_cast<py::ssize_t>(n)), oy(static_cast<py::ssize_t>(n));
        Status s;
        {
            py::gil_scoped_release nogil;
            s = transform_xy(src, dst, static_cast<const double*>(bx.ptr), static_cast<const double*>(by.ptr),
                             ox.mutable_data(), oy.mutable_data(), n, MemoryLocation::Host);
        }
        raise_if_error(s);
        return py::make_tuple(ox, oy);
    });
    // device arrays given by address, enqueued on `stream` (0: the null stream)
    m.def("_transform_xy_device", [](const CRS& src, const CRS& dst, uintptr_t x, uintptr_t y, uintptr_t ox, uintptr_t oy,
                                     size_t n, uintptr_t stream) {
        pcr_hip_crs_desc s, d;
        raise_if_error(detail::crs_desc(src, "source", &s));
        raise_if_error(detail::crs_desc(dst, "destination", &d));
        const int rc = pcr_hip_transform_xy(&s, &d, reinterpret_cast<const double*>(x), reinterpret_cast<const double*>(y),
                                            reinterpret_cast<double*>(ox), reinterpret_cast<double*>(oy), n,
                                            reinterpret_cast<void*>(stream));
        if (rc != PCR_HIP_OK) throw std::runtime_error(pcr_hip_last_error());
    });
    m.def("reproject", [](PointCloud& cloud, const CRS& dst) {
        Status s;
        {
            py::gil_scoped_release nogil;
            s = reproject(cloud, dst);
        }
        raise_if_error(s);
    }, py::arg("cloud"), py::arg("dst_crs"), "Reprojects the cloud's x, y in place (Host, HostPinned or Device) and sets its CRS");
    // what Pipeline.ingest would do about this cloud's CRS: None (ingest it as it is) or the CRS it is reprojected into;
    // RuntimeError when it would refuse (pcr/distributed.py routes by x, y and decides first)
    m.def("_plan_reprojection", [](const PipelineConfig& cfg, const CRS& cloud_crs) -> py::object {
        std::unique_ptr<PointCloud> probe = PointCloud::create(1);
        probe->set_crs(cloud_crs);
        detail::Reprojection rp;
        raise_if_error(detail::plan_reprojection(cfg, *probe, &rp));
        if (!rp.needed) return py::none();
        return py::cast(rp.dst_crs);
    });

    // extension: a band sampled at the points of a cloud, where the cloud lives (a Device cloud: in HBM)
    py::enum_<SampleMode>(m, "SampleMode").value("Nearest", SampleMode::Nearest).value("Bilinear", SampleMode::Bilinear);
    m.def("sample_grid", [](PointCloud& cloud, const Grid& grid, int band, const std::string& channel, py::object value_channel,
                            SampleMode mode) {
        const std::string value = value_channel.is_none() ? std::string() : value_channel.cast<std::string>();
        Status s;
        {
            py::gil_scoped_release nogil;
            s = sample_grid(cloud, grid, band, channel, value, mode);
        }
        raise_if_error(s);
    }, py::arg("cloud"), py::arg("grid"), py::arg("band") = 0, py::arg("channel") = "sample", py::arg("value_channel") = py::none(),
       py::arg("mode") = SampleMode::Bilinear,
       "Adds (or overwrites) the Float32 channel `channel`: the band's sample at every point, or value_channel minus it");

    // extension: the terrain bands of a grid's band, where the grid lives (a Device grid: in HBM)
    m.def("terrain", [](const Grid& grid, int band, const std::vector<TerrainProduct>& products, py::object spec, double cell_size_x,
                        double cell_size_y) {
        Status s;
        auto out = terrain(grid, band, products, spec.is_none() ? TerrainSpec() : spec.cast<TerrainSpec>(), cell_size_x, cell_size_y,
                           &s, nullptr);
        raise_if_error(s);
        return out;
    }, py::arg("grid"), py::arg("band"), py::arg("products"), py::arg("spec") = py::none(), py::arg("cell_size_x") = 1.0,
       py::arg("cell_size_y") = -1.0);
    // extension: tree tops and crown labels of a grid's band, where the grid lives (a Device grid: in HBM)
    m.def("segment_trees", [](const Grid& grid, int band, py::object spec, double cell_size_x, double cell_size_y) {
        Status s;
        TreeTable t;
        auto out = segment_trees(grid, band, spec.is_none() ? TreeSpec() : spec.cast<TreeSpec>(), cell_size_x, cell_size_y, &t, &s, nullptr);
        raise_if_error(s);
        return py::make_tuple(std::move(out), tree_table_dict(t));
    }, py::arg("grid"), py::arg("band") = 0, py::arg("spec") = py::none(), py::arg("cell_size_x") = 1.0, py::arg("cell_size_y") = -1.0,
       "(grid with the bands tree_id and tree_height, table): the table a dict of numpy arrays row, col, x, y, height, crown_cells");
    // extension: polygons burnt into a label grid (pcr.rasterize_polygons, Pipeline.set_zones)
    using F64Array = py::array_t<double, py::array::c_style | py::array::forcecast>;
    using I64Array = py::array_t<int64_t, py::array::c_style | py::array::forcecast>;
    py::class_<PolygonSet>(m, "PolygonSet",
                           "P polygons of R rings of V vertices: coords (V, 2) float64, ring_offsets (R + 1) and polygon_offsets (P + 1) "
                           "int64, values (P) float32 or None for p + 1.  Rings close implicitly; a polygon is all of its rings under the "
                           "even-odd rule")
        .def(py::init([](F64Array coords, I64Array ring_offsets, I64Array polygon_offsets, py::object values) {
            if (!((coords.ndim() == 2 && coords.shape(1) == 2) || coords.size() == 0))
                throw std::invalid_argument("PolygonSet: coords must have the shape (V, 2)");
            if (ring_offsets.ndim() != 1 || polygon_offsets.ndim() != 1) throw std::invalid_argument("PolygonSet: offsets must be 1-D");
            PolygonSet s;
            s.coords.assign(coords.data(), coords.data() + coords.size());
            s.ring_offsets.assign(ring_offsets.data(), ring_offsets.data() + ring_offsets.size());
            s.polygon_offsets.assign(polygon_offsets.data(), polygon_offsets.data() + polygon_offsets.size());
            if (!values.is_none()) {
                auto v = values.cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
                if (v.ndim() != 1 || v.size() + 1 != polygon_offsets.size()) throw std::invalid_argument("PolygonSet: values must be one per polygon");
                s.values.assign(v.data(), v.data() + v.size());
            }
            return s;
        }), py::arg("coords"), py::arg("ring_offsets"), py::arg("polygon_offsets"), py::arg("values") = py::none())
        .def_property_readonly("coords", [](const PolygonSet& s) {
            py::array_t<double> a({(py::ssize_t)s.num_vertices(), (py::ssize_t)2});
            if (!s.coords.empty()) std::memcpy(a.mutable_data(), s.coords.data(), s.coords.size() * sizeof(double));
            return a;
        })
        .def_property_readonly("ring_offsets", [](const PolygonSet& s) {
            return py::array_t<int64_t>((py::ssize_t)s.ring_offsets.size(), s.ring_offsets.data());
        })
        .def_property_readonly("polygon_offsets", [](const PolygonSet& s) {
            return py::array_t<int64_t>((py::ssize_t)s.polygon_offsets.size(), s.polygon_offsets.data());
        })
        .def_property_readonly("values", [](const PolygonSet& s) -> py::object {
            if (s.values.empty()) return py::none();
            return py::array_t<float>((py::ssize_t)s.values.size(), s.values.data());
        })
        .def_property_readonly("num_vertices", &PolygonSet::num_vertices)
        .def_property_readonly("num_rings", &PolygonSet::num_rings)
        .def_property_readonly("num_polygons", &PolygonSet::num_polygons);
    m.def("rasterize_polygons", [](const PolygonSet& polygons, const GridConfig& grid_config, float background, MemoryLocation location) {
        Status s;
        RasterizeOptions o;
        o.background = background;
        auto out = rasterize_polygons(polygons, grid_config, location, o, &s, nullptr);
        raise_if_error(s);
        return out;
    }, py::arg("polygons"), py::arg("grid_config"), py::arg("background") = std::numeric_limits<float>::quiet_NaN(),
       py::arg("location") = MemoryLocation::Host,
       "A one-band Float32 grid 'label' on grid_config at `location`: per cell the value of the greatest-index polygon that holds the "
       "cell's centre (p + 1, or the set's values), `background` elsewhere");
    // extension: the exact per-point test (pcr.points_in_polygons)
    m.def("points_in_polygons", [](PointCloud& cloud, const PolygonSet& polygons, const std::string& channel, float background,
                                   int index_cols, int index_rows) {
        PointInPolygonOptions o;
        o.background = background;
        o.index_cols = index_cols;
        o.index_rows = index_rows;
        Status s;
        {
            py::gil_scoped_release nogil;
            s = points_in_polygons(cloud, polygons, channel, o);
        }
        raise_if_error(s);
    }, py::arg("cloud"), py::arg("polygons"), py::arg("channel") = "polygon",
       py::arg("background") = std::numeric_limits<float>::quiet_NaN(), py::arg("index_cols") = 0, py::arg("index_rows") = 0,
       "Adds (or overwrites) the Float32 channel `channel`: per point the value of the greatest-index polygon that holds the point "
       "(p + 1, or the set's values), `background` elsewhere -- exact, where a label grid sampled Nearest gives the cell's");
    // extension: the other way round, the zones of a band as polygons (pcr.polygonize, Pipeline.polygonize)
    m.def("polygonize", [](const Grid& grid, int band, py::object grid_config) {
        Status s;
        GridConfig g;
        if (!grid_config.is_none()) g = grid_config.cast<GridConfig>();
        PolygonSet out = polygonize(grid, band, grid_config.is_none() ? nullptr : &g, &s, nullptr);
        raise_if_error(s);
        return out;
    }, py::arg("grid"), py::arg("band") = 0, py::arg("grid_config") = py::none(),
       "The zones of a band (whole numbers in [1, 2^24]) as a PolygonSet, made where the grid lives: one polygon per zone by "
       "ascending zone, its value the zone, its rings the 4-connected outlines under the even-odd rule, on grid_config or the "
       "grid's own geometry");
    // (tests) what the id band holds for an id: the clamp at 2^24 on its own
    m.def("_tree_id_value", [](int64_t id) { return pcrhip::trees::id_value(id); }, py::arg("id"));
    // (tests, tools) the host twin on an array, which the kernels are compared with; -> (id [h, w], height [h, w], table)
    m.def("_trees_host", [](py::array_t<float, py::array::c_style | py::array::forcecast> src, py::object spec_in, double cell_size_x,
                            double cell_size_y) {
        if (src.ndim() != 2 || src.shape(0) < 1 || src.shape(1) < 1) throw std::invalid_argument("segment_trees: a 2-D array is needed");
        const TreeSpec spec = spec_in.is_none() ? TreeSpec() : spec_in.cast<TreeSpec>();
        const std::string bad = detail::tree_spec_error(spec);
        if (!bad.empty()) throw std::invalid_argument("segment_trees: " + bad);
        if (!detail::tree_cell_sizes_ok(cell_size_x, cell_size_y)) throw std::invalid_argument("segment_trees: cell sizes must be finite and not zero");
        const int h = (int)src.shape(0), w = (int)src.shape(1);
        py::array_t<float> id({(py::ssize_t)h, (py::ssize_t)w}), height({(py::ssize_t)h, (py::ssize_t)w});
        TreeTable t;
        raise_if_error(detail::trees_host(src.data(), w, h, w, detail::tree_consts(spec, cell_size_x, cell_size_y), id.mutable_data(), w,
                                          height.mutable_data(), w, &t));
        detail::tree_centres(t, nullptr, cell_size_x, cell_size_y);
        return py::make_tuple(id, height, tree_table_dict(t));
    }, py::arg("src"), py::arg("spec") = py::none(), py::arg("cell_size_x") = 1.0, py::arg("cell_size_y") = -1.0);
    // (tests, tools) the host loop on an array, which the kernel is compared with; -> [len(products), h, w]
    m.def("_terrain_host", [](py::array_t<float, py::array::c_style | py::array::forcecast> src, const std::vector<TerrainProduct>& products,
                              py::object spec_in, double cell_size_x, double cell_size_y, int threads) {
        if (src.ndim() != 2 || src.shape(0) < 1 || src.shape(1) < 1) throw std::invalid_argument("terrain: a 2-D array is needed");
        const TerrainSpec spec = spec_in.is_none() ? TerrainSpec() : spec_in.cast<TerrainSpec>();
        const std::string bad = detail::terrain_spec_error(spec);
        if (!bad.empty()) throw std::invalid_argument("terrain: " + bad);
        if (!detail::terrain_cell_sizes_ok(cell_size_x, cell_size_y)) throw std::invalid_argument("terrain: cell sizes must be finite and not zero");
        unsigned mask = 0;
        std::vector<int> ids;
        for (TerrainProduct p : products) {
            if (!terrain_product_name(p)[0] || (mask & (1u << (int)p))) throw std::invalid_argument("terrain: unknown or duplicate product");
            mask |= 1u << (int)p;
            ids.push_back((int)p);
        }
        if (ids.empty()) throw std::invalid_argument("terrain: no product asked for");
        const int h = (int)src.shape(0), w = (int)src.shape(1);
        py::array_t<float> out({(py::ssize_t)ids.size(), (py::ssize_t)h, (py::ssize_t)w});
        std::vector<float*> dsts;
        std::vector<int64_t> strides;
        for (size_t k = 0; k < ids.size(); ++k) {
            dsts.push_back(out.mutable_data() + k * (size_t)h * w);
            strides.push_back(w);
        }
        const int before = omp_get_max_threads();
        if (threads > 0) omp_set_num_threads(threads);
        detail::terrain_host(src.data(), w, h, w, (int)ids.size(), ids.data(), dsts.data(), strides.data(),
                             detail::terrain_consts(spec, cell_size_x, cell_size_y), spec.compute_edges ? 1 : 0);
        omp_set_num_threads(before);
        return out;
    }, py::arg("src"), py::arg("products"), py::arg("spec") = py::none(), py::arg("cell_size_x") = 1.0, py::arg("cell_size_y") = -1.0,
       py::arg("threads") = 0);
}
