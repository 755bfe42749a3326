// device_pipeline.h -- (internal) Pipeline::Impl: the in-core pipeline on the HIP engine.  State planes in grid layout,
// resident in HBM for the pipeline's life; every device action goes through the C-ABI of include/pcr_hip.h.
// The rules about who may trust the planes, the touched flags and the stored bands are in device_pipeline.cpp, "plane state".
#pragma once

#include "buffer.h"
#include "cell_stats.h"
#include "extremes.h"
#include "ground_filter.h"
#include "histogram.h"
#include "pcr/core/grid.h"
#include "pcr/engine/pipeline.h"
#include "pipeline_common.h"
#include "point_zonal.h"
#include "polygons.h"
#include "sample_grid.h"
#include "terrain.h"
#include "trees.h"
#include "zonal.h"

#include <chrono>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace pcr {

struct Pipeline::Impl {
    struct Group : detail::GroupSpec {   // one pass over the points (detail::plan_groups) and what this engine keeps for it
        detail::Buffer planes[4];
        pcr_hip_planes view{};
        // A MostRecent group (select): its state on the device is ONE plane of packed 64-bit words (`packed`, 8 B per
        // cell, include/pcr_hip.h "MostRecent").  mask names slots 0 / 1, the two float planes (value, timestamp) the state is
        // at the host-visible boundary: planes[0] / planes[1] only exist while a checkpoint, a parked band or a shard's
        // state_planes() needs that view (select_unpack / select_pack).
        detail::Buffer packed;
        bool fresh = true;               // nothing has been accumulated yet: the first Point merge may store
        bool defined = false;            // the planes hold values (identity or accumulated).  They are NOT filled at create:
                                         // the first scatter defines them inside ingest, as the reference initialises its tile
                                         // state inside ingest (pipeline.cpp:688-691) -- see define_planes()
        bool bands_with_scatter = false; // the scatter that defined the planes was asked to store this group's finished bands
                                         // too (pcr_hip_engine_finalize_with_scatter) and nothing has touched the planes or the
                                         // touched flags since: finalize() skips the group's kernel when the device agrees
        uint32_t planes_in_bands = 0;    // PCR_HIP_PLANE_* bits of planes that scatter did NOT store (pcr_hip_engine_defer_planes):
                                         // where the group's done word reads 1 their memory is undefined and their values are
                                         // in the band of their own reduction -- restore_planes() puts them back in front of
                                         // everything that reads or writes the planes or the touched flags, finalize apart.
                                         // Non-zero only while bands_with_scatter is true.  Relies on the bands being the
                                         // pipeline's alone to write: result() hands out a const Grid*, result_band_device() a
                                         // const float*.
    };
    using Output = detail::Output;
    // What the steps of one ingest share.
    struct Ingest {
        const PointCloud& cloud;
        size_t n;
        const void *dx = nullptr, *dy = nullptr;             // the coordinates every kernel reads (reprojected when need be)
        std::map<std::string, const float*> staged;          // a channel is staged once per ingest, whoever asks first
        detail::ChannelLookup channel;                       // Impl::channel_of over `staged`
        std::vector<const uint8_t*> class_mask;              // the filter stage's masks, per class (detail::sweep_filter_classes)
        size_t kept = 0;                                     // PipelineConfig::filter's survivors
    };

    // The pipeline's device is made current for the duration of a call that launches or allocates, whatever the
    // calling thread had current (torch, another pipeline).
    struct DeviceScope {
        int prev = -1;
        bool changed = false;
        explicit DeviceScope(int dev) {
            if (pcr_hip_get_device(&prev) == PCR_HIP_OK && prev != dev) changed = pcr_hip_set_device(dev) == PCR_HIP_OK;
        }
        ~DeviceScope() { if (changed) pcr_hip_set_device(prev); }
        DeviceScope(const DeviceScope&) = delete;
        DeviceScope& operator=(const DeviceScope&) = delete;
    };

    PipelineConfig cfg;
    ProgressCallback callback;
    pcr_hip_grid hg{};
    pcr_hip_engine* engine = nullptr;
    pcr_hip_stream stream = nullptr;
    bool own_stream = false;
    std::vector<Group> groups;
    std::vector<Output> outputs;
    // Which memory a band is.  One row per band of the result grid -- the outputs, then the DTM, then the hag band, then the
    // terrain bands, then the tree bands -- built once by allocate_result(); everything else only reads it.  A band is FILLED iff
    // fill_nodata_radius > 0 and it is an output with fills_nodata(type), or it is the DTM; the hag band, the terrain bands and the tree
    // bands never are.  Device result: `out` is the result grid's
    // band, `raw` is `out` unless the band is filled, then an owned buffer.  Host result: `raw` is an owned buffer, `out` is
    // `raw` unless the band is filled, then a second owned buffer.  The fill and the ground filter read a raw band and write
    // another buffer, so the raw bands stay what the plane-state rules take them for: the table is no plane-state event.
    struct LeavingBand {
        float* raw = nullptr;                // device: what the finalize kernels, a defining scatter or the ground filter store;
                                             // for an output, also what carries its deferred planes
        float* out = nullptr;                // device: the band as it leaves the pipeline: result(), result_band_device(), the
                                             // GeoTIFF and its overview levels (== raw unless it is filled)
    };
    std::vector<LeavingBand> bands;
    std::vector<detail::Buffer> band_buffers;    // the owned buffers behind the table; a buffer's role is its place in the table
    detail::GroundPlan ground;               // PipelineConfig::ground, planned at init
    detail::Buffer d_ground_work;            // its workspace, allocated by the first finalize, grow-only
    detail::TerrainPlan terrain;             // PipelineConfig::terrain, planned at init
    detail::TreesPlan tree_plan;             // PipelineConfig::trees, planned at init
    std::vector<detail::Buffer> d_tree_work; // entry by entry: the work area of pcr_hip_trees, allocated by the first finalize,
                                             // grow-only; between a finalize and the next it holds the entry's tree count, ids
                                             // and crown counts, which trees() reads
    detail::ZonalPlan zonal_plan;            // PipelineConfig::zonal, planned at init
    std::map<std::string, detail::ZoneGrid> zone_grids;   // the label grids of set_zones, by name, in HBM
    bool zonal_fresh = false;                // the last finalize's bands and the planes belong together: no ingest since
    detail::PointZonalPlan pz_plan;          // PipelineConfig::point_zonal, planned at init
    detail::PointZonalState pz_state;        // its tables in HBM, zeroed at create and only ever added to, at every ingest: no part
                                             // in the plane-state rules
    detail::FilterPlan filters;              // PipelineConfig::filter (class 0) and every ReductionSpec::filter, planned at init
    detail::HistogramPlan hist;              // PipelineConfig::histograms, planned at init
    std::vector<detail::Buffer> cubes;       // entry by entry: count[bins][state_rows * width] in HBM, zeroed at create and only
                                             // ever added to: no part in the plane-state rules
    detail::ExtremesPlan ext;                // PipelineConfig::extremes, planned at init
    std::vector<detail::Buffer> ext_keys;    // entry by entry: keys[k][state_rows * width] in HBM, all EMPTY at create and only
                                             // ever lowered: no part in the plane-state rules
    detail::CellStatsPlan cstats;             // PipelineConfig::cell_stats, planned at init
    struct StatPlanes { detail::Buffer n, s1, s2; };
    std::vector<StatPlanes> stat_planes;     // entry by entry: N (uint32), S1 (int64), S2 (uint64) over state_rows * width in HBM,
                                             // zeroed at create and only ever added to: no part in the plane-state rules
    std::vector<detail::Surface> surfaces;   // PipelineConfig::surface_channels, entry by entry: the band in HBM (set_surface)
    detail::PolygonChannels polygon_sets;    // PipelineConfig::polygon_channels, entry by entry: the index, its tables in HBM (set_polygons)
    detail::Buffer d_bands_done;             // one word per group, set by a scatter that stored the group's bands.  Page-locked
                                             // host memory the device writes through its mapping (the pointer is the same on
                                             // both sides): the blocking finalize reads it after its synchronise and launches
                                             // nothing for a group whose bands are there
    bool state_shared = false;               // plane / touched-flag pointers have left the pipeline: never finalize with a scatter
    std::unique_ptr<Grid> result;
    bool finalized = false;                  // result() is null until the first finalize, as in the reference
    std::map<std::string, detail::Buffer> staging;   // by name, grow-only (staging_at_least alone touches it): device copies of
                                             // host-resident arrays, the reprojected x / y, the surface samples, the filter
                                             // stage's masks, the Line-reach words
    int halo = 0;
    size_t collections = 0;
    size_t points = 0;
    bool continue_on_host = false;           // init() failed where the reference carries on in CPU mode (see init)
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();

    ~Impl();

    // ---- what Pipeline's methods dispatch to
    Status init();
    Status ingest(const PointCloud& cloud, bool wait = true);
    Status finalize(bool wait = true);
    Status set_surface(const std::string& name, const Grid& grid, int band);
    Status set_polygons(const std::string& name, const PolygonSet& polygons, const PointInPolygonOptions& options);
    Status save_state(const std::string& dir);
    Status load_state(const std::string& dir);
    ProgressInfo stats() const;
    Status synchronize();
    Status query_line_reach(const PointCloud& cloud, int* rows_out);
    int state_row_begin() const { return hg.state_row0; }
    int state_row_count() const { return hg.state_rows; }
    std::vector<PlaneView> state_planes();
    std::vector<int> reduction_groups() const;
    void* tile_touched_device(int* tiles_x, int* tiles_y);
    const void* tile_touched_device_readonly(int* tiles_x, int* tiles_y) const;
    Status merge_touched(const void* d_union);
    const float* result_band_device(int band);
    void profile_enable(bool on, const std::string& only_kernel);
    std::vector<KernelTime> profile_read(bool reset);
    ScatterInfo last_scatter() const;
    // The state WINDOW of this pipeline (any shard) as host copies: planes[4 g + p] (state_rows x W floats; empty when group g
    // has no plane p) + the touched flags.  What the out-of-core driver parks between two visits of a band.
    Status export_window(std::vector<std::vector<float>>& planes, std::vector<uint32_t>& touched);
    Status import_window(const std::vector<std::vector<float>>& planes, const std::vector<uint32_t>& touched);

    // ---- plane state: every assignment to fresh / defined / bands_with_scatter / planes_in_bands / state_shared (see the .cpp)
    Status restore_planes(size_t gi, bool* enqueued = nullptr);
    Status restore_all_planes(bool* enqueued = nullptr);
    Status bands_stale();
    Status define_identity(Group& gr);
    Status define_planes(Group& gr);
    Status define_all_planes();
    int scatter_mode(const Group& gr) const;                 // event: planes about to be written by a scatter
    void scatter_done(Group& gr, bool offered, bool ok);     // event: a scatter finished
    void state_imported(Group& gr);                          // event: state imported from outside
    void planes_leave();                                     // event: plane pointers leave
    void flags_leave();                                      // event: the flag pointer leaves, writable
    void done_word_is_zero(Group& gr);                       // event: the host learns the done word is 0

    // ---- the rest
    int own_rows() const { return hg.own_row1 - hg.own_row0; }
    static int own_plane(ReductionType t);
    Status band_leaves(size_t b, bool* enqueued);
    Status finalize_histograms(bool* enqueued);
    Status histogram_counts(int i, std::vector<uint32_t>* out);
    Status finalize_extremes(bool* enqueued);
    Status extremes_values(int i, std::vector<float>* out);
    Status finalize_cell_stats(bool* enqueued);
    Status cell_stats_state(int i, std::vector<uint32_t>* n, std::vector<int64_t>* s1, std::vector<uint64_t>* s2);
    Status finalize_ground(bool* enqueued);
    Status finalize_terrain(bool* enqueued);
    Status finalize_trees(bool* enqueued);
    Status trees(int i, TreeTable* out);
    Status set_zones(const std::string& name, const Grid& grid, int band);
    Status set_zones(const std::string& name, const PolygonSet& polygons, const RasterizeOptions& options);
    Status zonal(int i, ZonalTable* out, bool with_counts);
    Status polygonize(const std::string& band_name, PolygonSet* out);
    Status point_zonal(int i, PointZonalTable* out, bool with_counts);
    Status touched_flags(uint32_t** d, int* tx = nullptr, int* ty = nullptr) const;
    bool offer_bands(size_t gi);
    Status unpack_select(Group& gr);
    Status alloc_select_views(Group& gr);
    Status pack_select(Group& gr);
    void drop_select_views();
    int reach_rows(const GlyphSpec& gl) const;
    bool block_is_whole_tiles() const;
    Status line_reach_rows(const GlyphSpec& gl, const void* d_half_length, const uint8_t* d_mask, size_t n, int* rows_needed);
    Status reach_error(int rows) const;
    Status staging_at_least(const std::string& key, size_t bytes, detail::Buffer** out);
    Status device_array(const void* src, MemoryLocation loc, size_t bytes, const std::string& key, const void** out);
    // ---- the steps of ingest(), in its order
    Status channel_of(Ingest& in, const std::string& name, const float** out);
    Status stage_xy(Ingest& in, const detail::Reprojection& rp);
    Status sample_surfaces(Ingest& in);
    Status locate_polygons(Ingest& in);
    Status filter_stage(Ingest& in);
    Status check_line_reach(Ingest& in);
    Status scatter_groups(Ingest& in);
    Status scatter_histograms(Ingest& in);
    Status scatter_extremes(Ingest& in);
    Status scatter_cell_stats(Ingest& in);
    Status fold_point_zonal(Ingest& in);
    Status marshal_glyph(const GlyphSpec& gl, const detail::ChannelLookup& channel, pcr_hip_glyph* out) const;
    Status allocate_result();
    Status checkpoint_dir(const std::string& dir_in, std::string* dir, bool writing) const;
    detail::StateWindow state_window(std::vector<std::vector<float>>& planes) const;
};

}  // namespace pcr
