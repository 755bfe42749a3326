// pipeline.cpp -- Pipeline::{create, ingest, finalize, ...}: the facade over the three engines -- the in-core device
// pipeline (device_pipeline.h), the out-of-core driver (banded_pipeline.h) and the host engine (host_pipeline.h).
//
// Same observable contract as the reference's src/engine/pipeline.cpp (validation and error
// strings :365-378, 500-508; empty cloud no-op :284-287; per-ingest progress callback and
// "cancelled by user" :753-767; band naming :1175-1186; NaN for untouched tiles :1204-1222;
// state survives finalize), but a different machine underneath:
//   * no router / sort / per-tile batches / tile manager: reductions that read the same value
//     channel through the same glyph share ONE pass over the points and ONE set of device
//     planes (sum, weight, max, min) in grid layout, resident in HBM for the pipeline's life;
//   * finalize runs on the device; only finalized bands cross PCIe (or stay in HBM);
//   * every device action goes through the C-ABI of include/pcr_hip.h.
#include "pcr/engine/pipeline.h"

#include "banded_pipeline.h"
#include "device_pipeline.h"
#include "ground_filter.h"
#include "cell_stats.h"
#include "extremes.h"
#include "histogram.h"
#include "terrain.h"
#include "trees.h"
#include "zonal.h"
#include "host_pipeline.h"
#include "las_io.h"
#include "pcr/core/point_cloud.h"
#include "pcr/io/point_cloud_io.h"
#include "point_zonal.h"
#include "polygons.h"
#include "sample_grid.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace pcr {

namespace {

thread_local std::string g_create_error;

// Every channel a configuration reads from its clouds: the reductions' value, weight, timestamp and glyph channels, their own
// filters' and the pipeline filter's -- what a LAS file is decoded into (a Pipeline never looks at any other).  A surface
// channel is derived, never read: its name is dropped and its value_channel added (`hag` alone decodes `z`).
std::vector<std::string> named_channels(const PipelineConfig& c) {
    std::vector<std::string> out;
    auto add = [&out, &c](const std::string& name) {
        if (name.empty() || detail::derived_channel(c, name)) return;
        if (std::find(out.begin(), out.end(), name) == out.end()) out.push_back(name);
    };
    for (const auto& r : c.reductions) {
        add(r.value_channel);
        add(r.weight_channel);
        add(r.timestamp_channel);
        add(r.glyph.direction_channel);
        add(r.glyph.half_length_channel);
        add(r.glyph.sigma_x_channel);
        add(r.glyph.sigma_y_channel);
        add(r.glyph.rotation_channel);
        for (const auto& p : r.filter.predicates) add(p.channel_name);
    }
    for (const auto& p : c.filter.predicates) add(p.channel_name);
    for (const auto& h : c.histograms) {
        add(h.value_channel);
        for (const auto& p : h.filter.predicates) add(p.channel_name);
    }
    for (const auto& e : c.extremes) {
        add(e.value_channel);
        for (const auto& p : e.filter.predicates) add(p.channel_name);
    }
    for (const auto& s : c.cell_stats) {
        add(s.value_channel);
        for (const auto& p : s.filter.predicates) add(p.channel_name);
    }
    for (const auto& z : c.point_zonal) {                    // (a LAS channel that only a point-zonal entry names is decoded too)
        add(z.label_channel);
        for (const auto& s : z.cell_stats) {
            add(s.value_channel);
            for (const auto& p : s.filter.predicates) add(p.channel_name);
        }
        for (const auto& h : z.histograms) {
            add(h.value_channel);
            for (const auto& p : h.filter.predicates) add(p.channel_name);
        }
    }
    for (const auto& sc : c.surface_channels) add(sc.value_channel);
    return out;
}

struct LasFd {
    int fd;
    explicit LasFd(const std::string& path) : fd(::open(path.c_str(), O_RDONLY)) {}
    ~LasFd() { if (fd >= 0) ::close(fd); }
    LasFd(const LasFd&) = delete;
    LasFd& operator=(const LasFd&) = delete;
};

}  // namespace

const std::string& pipeline_create_error() { return g_create_error; }

Pipeline::~Pipeline() = default;

bool Pipeline::out_of_core() const { return banded_ != nullptr; }

std::unique_ptr<Pipeline> Pipeline::create(const PipelineConfig& config) {
    auto p = std::unique_ptr<Pipeline>(new Pipeline());
    auto fail_with = [](const Status& s) {
        g_create_error = s.message;
        std::fprintf(stderr, "Error: %s\n", s.message.c_str());    // loud: there is no fallback path
        return std::unique_ptr<Pipeline>();
    };
    if (config.fill_nodata_radius < 0 || config.fill_nodata_radius > 32)
        return fail_with(Status::error(StatusCode::InvalidArgument, "pipeline: fill_nodata_radius must be between 0 and 32"));
    if (config.fill_nodata_radius > 0 && (config.shard_row_begin >= 0 || config.shard_row_end >= 0))
        return fail_with(Status::error(StatusCode::InvalidArgument,
            "pipeline: fill_nodata_radius needs the whole grid; fill the gathered grid with fill_nodata"));
    {
        const Status hs = detail::check_histograms(config);     // (ahead of the ground and terrain plans, which may name its bands)
        if (!hs.ok()) return fail_with(hs);
        const Status es = detail::check_extremes(config);       // (likewise)
        if (!es.ok()) return fail_with(es);
        const Status cs = detail::check_cell_stats(config);     // (likewise)
        if (!cs.ok()) return fail_with(cs);
    }
    {
        detail::GroundPlan plan;                      // (every engine plans again for itself: here only the refusals)
        const Status gs = detail::plan_ground(config, &plan);
        if (!gs.ok()) return fail_with(gs);
        detail::TerrainPlan terrain;
        const Status ts = detail::plan_terrain(config, plan, &terrain);
        if (!ts.ok()) return fail_with(ts);
        detail::TreesPlan trees;
        const Status rs = detail::plan_trees(config, plan, terrain, &trees);
        if (!rs.ok()) return fail_with(rs);
        detail::ZonalPlan zonal;
        const Status zs = detail::plan_zonal(config, plan, terrain, trees, &zonal);
        if (!zs.ok()) return fail_with(zs);
    }
    {
        detail::FilterPlan filters;                   // (every engine plans again for itself: here only the refusals)
        detail::PointZonalPlan pz;
        Status zs = detail::plan_filters(config, &filters);
        if (zs.ok()) zs = detail::plan_point_zonal(config, filters, &pz);
        if (!zs.ok()) return fail_with(zs);
    }
    {
        const Status ss = detail::plan_surfaces(config);
        if (!ss.ok()) return fail_with(ss);
        const Status ps = detail::plan_polygon_channels(config);
        if (!ps.ok()) return fail_with(ps);
    }
    size_t budget = 0;
    if (Banded::needed(config, &budget)) {
        if (!config.point_zonal.empty()) return fail_with(detail::point_zonal_out_of_core_error());     // (its tables count: first)
        if (!config.surface_channels.empty()) return fail_with(detail::surfaces_out_of_core_error());
        if (!config.polygon_channels.empty()) return fail_with(detail::polygon_channels_out_of_core_error());
        if (!config.histograms.empty()) return fail_with(detail::histograms_out_of_core_error());
        if (!config.extremes.empty()) return fail_with(detail::extremes_out_of_core_error());
        if (!config.cell_stats.empty()) return fail_with(detail::cell_stats_out_of_core_error());
        if (!config.zonal.empty()) return fail_with(detail::zonal_out_of_core_error());
        Status bs = Status::success();
        p->banded_ = Banded::create(config, p.get(), budget, &bs);
        if (!p->banded_) return fail_with(bs);
        g_create_error.clear();
        return p;
    }
    auto on_host = [&]() -> std::unique_ptr<Pipeline> {
        p->impl_.reset();
        p->host_ = std::make_unique<Host>();
        p->host_->cfg = config;
        Status hs = p->host_->init();
        if (hs.ok() && config.resume && !config.state_dir.empty()) hs = p->host_->load_state(config.state_dir);
        if (!hs.ok()) return fail_with(hs);
        g_create_error.clear();
        return std::move(p);
    };
    if (config.exec_mode == ExecutionMode::CPU) return on_host();       // "CPU mode should always work" (tests/cpp/test_error_handling.cpp:181-199)
    p->impl_ = std::make_unique<Impl>();
    p->impl_->cfg = config;
    Status s = p->impl_->init();
    if (!s.ok() && p->impl_->continue_on_host) {
        // the reference's Warning / Info line is on stderr already (Impl::init)
        const char* forbid = std::getenv("PCR_REQUIRE_GPU_ENGINE");
        if (forbid && forbid[0] && forbid[0] != '0') return fail_with(s);
        return on_host();
    }
    if (s.ok() && config.resume && !config.state_dir.empty()) s = p->impl_->load_state(config.state_dir);
    if (!s.ok()) return fail_with(s);
    g_create_error.clear();
    return p;
}

const char* Pipeline::engine() const { return host_ ? "host" : "hip"; }
int Pipeline::host_threads() const { return host_ && host_->engine ? host_->engine->threads() : 0; }
std::string Pipeline::spill_dir() const { return banded_ ? banded_->spill_dir : std::string(); }

Status Pipeline::validate() const {
    const PipelineConfig& c = host_ ? host_->cfg : banded_ ? banded_->cfg : impl_->cfg;
    if (c.grid.width <= 0 || c.grid.height <= 0)
        return Status::error(StatusCode::InvalidArgument, "pipeline: grid dimensions must be positive");
    if (c.grid.tile_width <= 0 || c.grid.tile_height <= 0)
        return Status::error(StatusCode::InvalidArgument, "pipeline: tile dimensions must be positive");
    if (c.reductions.empty())
        return Status::error(StatusCode::InvalidArgument, "pipeline: at least one reduction must be specified");
    for (const auto& r : c.reductions) {
        if (r.value_channel.empty())
            return Status::error(StatusCode::InvalidArgument, "pipeline: value_channel must be specified");
    }
    return detail::check_reduction_specs(c.reductions);
}

Status Pipeline::ingest(const PointCloud& cloud) { return host_ ? host_->ingest(cloud) : banded_ ? banded_->ingest(cloud) : impl_->ingest(cloud); }
Status Pipeline::ingest_async(const PointCloud& cloud) {
    return host_ ? host_->ingest(cloud) : banded_ ? banded_->ingest(cloud) : impl_->ingest(cloud, false);
}

Status Pipeline::ingest_file(const std::string& path, size_t chunk_points, size_t* points_read) {
    if (points_read) *points_read = 0;
    if (chunk_points == 0) return Status::error(StatusCode::InvalidArgument, "pipeline: chunk_points must be positive");
    const PipelineConfig& cfg = host_ ? host_->cfg : banded_ ? banded_->cfg : impl_->cfg;
    LasOptions las;                                          // (only a LAS file looks at it)
    las.channels = named_channels(cfg);
    las.gps_time_origin = cfg.las_gps_time_origin;
    Status opened;
    auto reader = PointCloudReader::open(path, PointCloudFormat::Auto, &las, &opened);
    if (!reader)
        return Status::error(opened.ok() ? StatusCode::IoError : opened.code,
                             "pipeline: failed to open point cloud file: " + path + (opened.message.empty() ? "" : ": " + opened.message));
    // The plain HIP engine takes a LAS file as raw records (the host engine and the out-of-core driver read it through the
    // reader and the host decoder, below)
    if (impl_ && reader->format() == PointCloudFormat::LAS) {
        reader.reset();
        return ingest_las_records(path, las, chunk_points, points_read);
    }
    chunk_points = std::min(chunk_points, std::max<size_t>(reader->info().num_points, 1));
    const MemoryLocation where = host_ ? MemoryLocation::Host : MemoryLocation::HostPinned;    // (no device: no page-locking either)
    std::unique_ptr<PointCloud> buf[2] = {PointCloud::create(chunk_points, where), PointCloud::create(chunk_points, where)};
    if (!buf[0] || !buf[1]) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate page-locked chunk buffers");
    for (auto& b : buf) b->set_crs(reader->info().crs);      // the file's CRS: ingest reprojects the chunks when it differs from the grid's
    size_t total = 0;
    int cur = 0;
    size_t got = reader->read_chunk(*buf[cur], chunk_points);
    while (got > 0) {
        Status s = ingest_async(*buf[cur]);              // H2D + kernels of this chunk, enqueued
        if (!s.ok()) { (void)synchronize(); return s; }
        total += got;
        got = reader->read_chunk(*buf[cur ^ 1], chunk_points);   // overlaps with them
        if (!(s = synchronize()).ok()) return s;         // buf[cur] is free again
        cur ^= 1;
    }
    if (points_read) *points_read = total;
    return Status::success();
}
// A LAS file on the HIP engine.  The loop of ingest_file with other buffers: two page-locked buffers of raw records, two
// device record buffers and two Device clouds that hold only the wanted channels.  Per chunk: one read, one asynchronous
// host-to-device copy, the decode kernel, then the ingest of the Device cloud -- all on the pipeline's stream, so the decode
// is ordered before the scatter that reads its output and after the previous scatter that read the same cloud (and nothing
// of chunk k is reused before the synchronize() that follows the read of chunk k + 1).  A format-1 record is 28 bytes: no
// more crosses PCIe than the decoded x, y and three channels would.
Status Pipeline::ingest_las_records(const std::string& path, const LasOptions& options, size_t chunk_points, size_t* points_read) {
    LasFd file(path);
    las::Header h;
    unsigned want = 0;
    Status s = las::read_header(file.fd, path, &h);
    if (s.ok()) s = las::wanted_mask(h, options.channels, &want);
    if (!s.ok()) return s;
    const pcr_hip_las_layout layout = h.layout(options.gps_time_origin);
    const size_t n = (size_t)h.num_points, len = h.record_length;
    if (n == 0) return Status::success();
    chunk_points = std::min(chunk_points, n);
    Impl::DeviceScope dev(impl_->cfg.cuda_device_id);
    detail::Buffer pinned[2], d_records[2];
    std::unique_ptr<PointCloud> cloud[2];
    float* out[2][PCR_HIP_LAS_CH_COUNT] = {};
    for (int b = 0; b < 2; ++b) {
        // + 16: the decode kernel stages with aligned 16-byte loads, the last of which may reach past the last record
        if (!(s = pinned[b].allocate(chunk_points * len + 16, MemoryLocation::HostPinned)).ok()) return s;
        if (!(s = d_records[b].allocate(chunk_points * len + 16, MemoryLocation::Device)).ok()) return s;
        cloud[b] = PointCloud::create(chunk_points, MemoryLocation::Device);
        if (!cloud[b]) return Status::error(StatusCode::OutOfMemory, "pipeline: failed to allocate device chunk clouds");
        cloud[b]->set_crs(h.crs);                            // the file's CRS: ingest reprojects the chunks when it differs from the grid's
        for (int c = 0; c < PCR_HIP_LAS_CH_COUNT; ++c) {
            if (!(want & (1u << c))) continue;
            if (!(s = cloud[b]->add_channel(las::kChannelNames[c], DataType::Float32)).ok()) return s;
            out[b][c] = cloud[b]->channel_f32(las::kChannelNames[c]);
        }
    }
    auto read_chunk = [&](int b, size_t first) -> size_t {  // records [first, ...) -> pinned[b]; 0 at the end or on a failed read
        if (first >= n) return 0;
        const size_t count = std::min(chunk_points, n - first);
        if (!las::read_bytes(file.fd, pinned[b].data(), count * len, h.data_offset + (uint64_t)first * len)) {
            s = Status::error(StatusCode::IoError, "pipeline: failed to read the point records of " + path);
            return 0;
        }
        return count;
    };
    size_t total = 0;
    int cur = 0;
    size_t got = read_chunk(cur, 0);
    while (got > 0) {
        Status e = cloud[cur]->resize(got);
        if (e.ok()) e = detail::hip_status(pcr_hip_memcpy_h2d(d_records[cur].data(), pinned[cur].data(), got * len, impl_->stream));
        if (e.ok()) e = detail::hip_status(pcr_hip_las_decode(&layout, static_cast<const uint8_t*>(d_records[cur].data()), got,
                                                              cloud[cur]->x(), cloud[cur]->y(), out[cur], impl_->stream));
        if (e.ok()) e = ingest_async(*cloud[cur]);           // kernels of this chunk, enqueued
        if (!e.ok()) { (void)synchronize(); return e; }
        total += got;
        got = read_chunk(cur ^ 1, total);                    // overlaps with them
        if (!(e = synchronize()).ok()) return e;             // the buffers of `cur` are free again
        cur ^= 1;
    }
    if (points_read) *points_read = total;
    return s;
}
Status Pipeline::set_polygons(const std::string& name, const PolygonSet& polygons, const PointInPolygonOptions& options) {
    if (host_) return host_->set_polygons(name, polygons, options);
    if (banded_) return Status::error(StatusCode::InvalidArgument, "pipeline: set_polygons: '" + name + "' names no polygon channel of this pipeline");
    return impl_->set_polygons(name, polygons, options);
}

Status Pipeline::set_surface(const std::string& name, const Grid& grid, int band) {
    if (host_) return host_->set_surface(name, grid, band);
    if (banded_) return Status::error(StatusCode::InvalidArgument, "pipeline: set_surface: '" + name + "' names no surface channel of this pipeline");
    return impl_->set_surface(name, grid, band);
}
Status Pipeline::histogram_counts(int i, std::vector<uint32_t>* out) const {
    if (impl_) return impl_->histogram_counts(i, out);
    if (!host_ || i < 0 || (size_t)i >= host_->cubes.size() || !out)
        return Status::error(StatusCode::InvalidArgument, "pipeline: histogram_counts: no histogram " + std::to_string(i));
    *out = host_->cubes[(size_t)i];
    return Status::success();
}
Status Pipeline::histogram_shape(int i, int* bins, int* rows, int* width) const {
    const PipelineConfig* c = host_ ? &host_->cfg : impl_ ? &impl_->cfg : nullptr;
    if (!c || i < 0 || (size_t)i >= c->histograms.size() || !bins || !rows || !width)
        return Status::error(StatusCode::InvalidArgument, "pipeline: histogram_counts: no histogram " + std::to_string(i));
    *bins = c->histograms[(size_t)i].bins;
    *rows = c->grid.height;                                  // (a row-block shard is refused: the window is the grid)
    *width = c->grid.width;
    return Status::success();
}
Status Pipeline::extremes_values(int i, std::vector<float>* out) const {
    if (impl_) return impl_->extremes_values(i, out);
    if (!host_ || i < 0 || (size_t)i >= host_->ext_keys.size() || !out)
        return Status::error(StatusCode::InvalidArgument, "pipeline: extremes_values: no extremes entry " + std::to_string(i));
    const PipelineConfig& c = host_->cfg;
    const size_t cells = (size_t)c.grid.width * c.grid.height;
    out->assign(host_->ext.entries[(size_t)i].state_cells(cells), 0.0f);
    std::vector<float> band(cells);                          // (the twin writes the band too: dropped)
    return detail::extremes_band_host(host_->ext.entries[(size_t)i], host_->ext_keys[(size_t)i].data(), c.grid.width, c.grid.height,
                                      band.data(), out->data(), host_->engine->threads());
}
Status Pipeline::extremes_shape(int i, int* k, int* rows, int* width) const {
    const PipelineConfig* c = host_ ? &host_->cfg : impl_ ? &impl_->cfg : nullptr;
    if (!c || i < 0 || (size_t)i >= c->extremes.size() || !k || !rows || !width)
        return Status::error(StatusCode::InvalidArgument, "pipeline: extremes_values: no extremes entry " + std::to_string(i));
    *k = c->extremes[(size_t)i].k;
    *rows = c->grid.height;                                  // (a row-block shard is refused: the window is the grid)
    *width = c->grid.width;
    return Status::success();
}
Status Pipeline::cell_stats_state(int i, std::vector<uint32_t>* n, std::vector<int64_t>* s1, std::vector<uint64_t>* s2) const {
    if (impl_) return impl_->cell_stats_state(i, n, s1, s2);
    if (!host_ || i < 0 || (size_t)i >= host_->stat_planes.size() || !n || !s1 || !s2)
        return Status::error(StatusCode::InvalidArgument, "pipeline: cell_stats_state: no cell_stats entry " + std::to_string(i));
    *n = host_->stat_planes[(size_t)i].n;
    *s1 = host_->stat_planes[(size_t)i].s1;
    *s2 = host_->stat_planes[(size_t)i].s2;
    return Status::success();
}
Status Pipeline::cell_stats_shape(int i, int* rows, int* width) const {
    const PipelineConfig* c = host_ ? &host_->cfg : impl_ ? &impl_->cfg : nullptr;
    if (!c || i < 0 || (size_t)i >= c->cell_stats.size() || !rows || !width)
        return Status::error(StatusCode::InvalidArgument, "pipeline: cell_stats_state: no cell_stats entry " + std::to_string(i));
    *rows = c->grid.height;                                  // (a row-block shard is refused: the window is the grid)
    *width = c->grid.width;
    return Status::success();
}
Status Pipeline::trees(int i, TreeTable* out) const {
    if (impl_) return impl_->trees(i, out);
    const std::vector<TreeTable>& tables = host_ ? host_->tree_tables : banded_->tree_tables;
    const std::vector<Status>& status = host_ ? host_->tree_status : banded_->tree_status;
    const bool finalized = host_ ? host_->finalized : banded_->finalized;
    if (!out || i < 0 || !finalized || (size_t)i >= tables.size())
        return Status::error(StatusCode::InvalidArgument, "pipeline: trees: no trees entry " + std::to_string(i) + " (of a finalize)");
    if (!status[(size_t)i].ok()) return status[(size_t)i];
    *out = tables[(size_t)i];
    return Status::success();
}
Status Pipeline::set_zones(const std::string& name, const Grid& grid, int band) {
    if (host_) return host_->set_zones(name, grid, band);
    if (banded_) return Status::error(StatusCode::InvalidArgument, "pipeline: set_zones: '" + name + "' names no external label grid of this pipeline");
    return impl_->set_zones(name, grid, band);
}
Status Pipeline::set_zones(const std::string& name, const PolygonSet& polygons, const RasterizeOptions& options) {
    if (host_) return host_->set_zones(name, polygons, options);
    if (banded_) return Status::error(StatusCode::InvalidArgument, "pipeline: set_zones: '" + name + "' names no external label grid of this pipeline");
    return impl_->set_zones(name, polygons, options);
}
Status Pipeline::zonal(int i, ZonalTable* out, bool with_counts) const {
    if (impl_) return impl_->zonal(i, out, with_counts);
    if (host_) return host_->zonal(i, out, with_counts);
    return Status::error(StatusCode::InvalidArgument, "pipeline: zonal: no zonal entry " + std::to_string(i) + " (of a finalize with no ingest since)");
}
Status Pipeline::point_zonal(int i, PointZonalTable* out, bool with_counts) const {
    if (impl_) return impl_->point_zonal(i, out, with_counts);
    if (host_) return host_->point_zonal(i, out, with_counts);
    return Status::error(StatusCode::InvalidArgument, "pipeline: point_zonal: no point_zonal entry " + std::to_string(i));
}
Status Pipeline::polygonize(const std::string& band_name, PolygonSet* out) const {
    if (impl_) return impl_->polygonize(band_name, out);
    if (host_) return host_->polygonize(band_name, out);
    return Status::error(StatusCode::InvalidArgument, "pipeline: polygonize: not on an out-of-core pipeline");
}
Status Pipeline::finalize() { return host_ ? host_->finalize() : banded_ ? banded_->finalize() : impl_->finalize(); }
Status Pipeline::finalize_async() { return host_ ? host_->finalize() : banded_ ? banded_->finalize() : impl_->finalize(false); }

Status Pipeline::run(const std::vector<const PointCloud*>& clouds) {
    for (const PointCloud* c : clouds) {
        if (!c) return Status::error(StatusCode::InvalidArgument, "pipeline: null cloud pointer");
        Status s = ingest(*c);
        if (!s.ok()) return s;
    }
    return finalize();
}

void Pipeline::set_progress_callback(ProgressCallback cb) {
    if (host_) host_->callback = std::move(cb);
    else if (banded_) banded_->callback = std::move(cb);
    else impl_->callback = std::move(cb);
}
const Grid* Pipeline::result() const {
    if (host_) return host_->finalized ? host_->result.get() : nullptr;
    if (banded_) return banded_->finalized ? banded_->result.get() : nullptr;
    return impl_->finalized ? impl_->result.get() : nullptr;
}
ProgressInfo Pipeline::stats() const { return host_ ? host_->stats() : banded_ ? banded_->stats() : impl_->stats(); }

// (out of core: no plane lives in HBM between two calls -- the shard accessors answer for "no shard")
int Pipeline::halo_rows() const { return banded_ || host_ ? 0 : impl_->halo; }
Status Pipeline::line_reach_rows(const PointCloud& cloud, int* rows) {
    if (banded_ || host_) { if (rows) *rows = 0; return Status::success(); }
    return impl_->query_line_reach(cloud, rows);
}
int Pipeline::state_row_begin() const { return banded_ || host_ ? 0 : impl_->state_row_begin(); }
int Pipeline::state_row_count() const { return banded_ || host_ ? 0 : impl_->state_row_count(); }

std::vector<Pipeline::PlaneView> Pipeline::state_planes() const {
    return banded_ || host_ ? std::vector<PlaneView>() : impl_->state_planes();
}
std::vector<int> Pipeline::reduction_groups() const { return banded_ || host_ ? std::vector<int>() : impl_->reduction_groups(); }
void* Pipeline::tile_touched_device(int* tiles_x, int* tiles_y) const {
    return banded_ || host_ ? nullptr : impl_->tile_touched_device(tiles_x, tiles_y);
}
const void* Pipeline::tile_touched_device_readonly(int* tiles_x, int* tiles_y) const {
    return banded_ || host_ ? nullptr : impl_->tile_touched_device_readonly(tiles_x, tiles_y);
}
Status Pipeline::merge_touched(const void* d_union) {
    if (banded_ || host_) return Status::error(StatusCode::NotImplemented, "pipeline: an out-of-core or host-engine pipeline is not a shard");
    return impl_->merge_touched(d_union);
}

Status Pipeline::save_state(const std::string& dir) {
    if (host_) return host_->save_state(dir);
    if (banded_) return banded_->save_state(dir);
    return impl_->save_state(dir);
}
Status Pipeline::load_state(const std::string& dir) {
    if (host_) return host_->load_state(dir);
    if (banded_) return banded_->load_state(dir);
    return impl_->load_state(dir);
}

const float* Pipeline::result_band_device(int band) const { return banded_ || host_ ? nullptr : impl_->result_band_device(band); }

Status Pipeline::synchronize() { return banded_ || host_ ? Status::success() : impl_->synchronize(); }
void* Pipeline::stream_handle() const { return banded_ || host_ ? nullptr : impl_->stream; }

void Pipeline::profile_enable(bool on, const std::string& only_kernel) {
    if (!banded_ && !host_) impl_->profile_enable(on, only_kernel);
}
std::vector<Pipeline::KernelTime> Pipeline::profile_read(bool reset) {
    return banded_ || host_ ? std::vector<KernelTime>() : impl_->profile_read(reset);
}
Pipeline::ScatterInfo Pipeline::last_scatter() const { return host_ ? host_->last : banded_ ? banded_->last : impl_->last_scatter(); }

}  // namespace pcr
