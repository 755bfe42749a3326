/*
 * pcr_hip.h -- C-ABI of libpcr_hip.so: the MI355X (gfx950) engine behind
 * pcr::Pipeline::ingest / finalize.
 *
 * Plain C: opaque handles, raw host/device pointers and sizes; no C++ or torch types.
 * Every function returns a pcr_hip_status (same numbering as the reference's
 * pcr::StatusCode, include/pcr/core/types.h:118-126; HIP failures map to
 * PCR_HIP_CUDA_ERROR to keep the reference's code name); the message of the last
 * failure on the calling thread is pcr_hip_last_error().
 *
 * The reference has no C ABI of its own.  Each entry point replaces one of its C++
 * seams, cited as "replaces:" (file:line into BigHippo123/pointcloud-raster).
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Layout conventions
 *   - points: SoA, x/y float64, channels float32 (include/pcr/core/point_cloud.h:29-103)
 *   - state:  band-sequential float32 planes in GRID layout, plane f at
 *             base + f*plane_stride, cell (row, col) at (row - state_row0)*width + col
 *             (the reference keeps per-tile planes, include/pcr/ops/reduction_op.h:45;
 *             tiles here are only a semantic: clip rectangle + "touched" flag)
 *   - all pointers named d_* are device pointers, h_* host pointers.
 */
#ifndef PCR_HIP_H
#define PCR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCR_HIP_ABI_VERSION 5   /* 3 (round 4): + comm_halo_plan / comm_agree_max_i32 / signed_max_f32_masked / copy_kernel; planes_fresh takes 0, 1, 2;
                                 * 4: + engine_finalize_with_scatter / engine_finalize_taken / finalize_group_unless / touched_union;
                                 * 5 (round 5): + comm_alltoall_counts / comm_alltoallv / comm_gatherv / comm_xfer_plan / touched_union_owned; halo_reduce resets the sent apron rows;
                                 *   later, additive (same version): + crs_from_epsg / transform_xy / transform_xy_host;
                                 *   + PCR_HIP_MOST_RECENT: select_pack / select_unpack / select_merge / scatter_select / finalize_select,
                                 *     state_floats / state_init / state_merge accept type 8;
                                 *   + engine_defer_planes / engine_planes_deferred / planes_from_bands_if; scatter_stats.reserved_ is now
                                 *     deferred_planes (same place, 0 unless the hint was sent);
                                 *   + las_decode / las_decode_host (LAS point records -> SoA cloud) */

typedef enum pcr_hip_status {
    PCR_HIP_OK = 0,
    PCR_HIP_INVALID_ARGUMENT = 1,
    PCR_HIP_OUT_OF_MEMORY = 2,
    PCR_HIP_CUDA_ERROR = 3,        /* a HIP runtime failure (name kept from the reference) */
    PCR_HIP_IO_ERROR = 4,
    PCR_HIP_CRS_ERROR = 5,
    PCR_HIP_NOT_IMPLEMENTED = 6
} pcr_hip_status;

/* pcr::ReductionType numbering (types.h:33-45).  The reference registers the first six
 * (src/ops/reduction_registry.cpp:173-184); MostRecent it only declares (builtin_ops.h:106-124): this build implements it
 * for the Point glyph through the pcr_hip_*select* entry points below.  The functions that take pcr_hip_planes refuse it. */
enum {
    PCR_HIP_SUM = 0, PCR_HIP_MAX = 1, PCR_HIP_MIN = 2,
    PCR_HIP_AVERAGE = 3, PCR_HIP_WEIGHTED_AVERAGE = 4, PCR_HIP_COUNT = 5,
    PCR_HIP_MOST_RECENT = 8
};

/* pcr::GlyphType numbering (include/pcr/engine/glyph.h:11-15). */
enum { PCR_HIP_GLYPH_POINT = 0, PCR_HIP_GLYPH_LINE = 1, PCR_HIP_GLYPH_GAUSSIAN = 2 };

/* Accumulation planes a scatter can feed in one pass over the points. */
enum {
    PCR_HIP_PLANE_SUM = 1u,   /* += value * w        (Sum; numerator of Average/WeightedAverage) */
    PCR_HIP_PLANE_WGT = 2u,   /* += w  (w = 1 for the Point glyph: Count; denominator)           */
    PCR_HIP_PLANE_MAX = 4u,   /* fmaxf, identity -FLT_MAX (Point glyph only)                      */
    PCR_HIP_PLANE_MIN = 8u    /* fminf, identity +FLT_MAX (Point glyph only)                      */
};

typedef void* pcr_hip_stream;      /* hipStream_t; NULL = the null stream */

/* The fields of pcr::GridConfig the hot path reads (include/pcr/core/grid_config.h:17-38)
 * plus the row window a device holds when the grid is row-block sharded over GPUs. */
typedef struct pcr_hip_grid {
    double min_x, min_y, max_x, max_y;   /* bounds; origin is (min_x, max_y) */
    double cell_size_x, cell_size_y;     /* cell_size_y < 0 on north-up grids */
    int32_t width, height;               /* whole grid, cells */
    int32_t tile_width, tile_height;     /* reference tiling (clip + touched semantics) */
    int32_t own_row0, own_row1;          /* this device ingests points whose centre row is in [own_row0, own_row1) */
    int32_t state_row0, state_rows;      /* rows held in the state planes: [state_row0, state_row0 + state_rows) */
} pcr_hip_grid;

/* Device planes of one accumulation group.  A NULL plane is not accumulated. */
typedef struct pcr_hip_planes {
    float* d_sum;
    float* d_wgt;
    float* d_max;
    float* d_min;
} pcr_hip_planes;

/* pcr::GlyphSpec numeric fields (glyph.h:20-42) + per-point channel arrays (device, may be NULL). */
typedef struct pcr_hip_glyph {
    int32_t type;
    float default_direction, default_half_length;
    float default_sigma_x, default_sigma_y, default_rotation;
    float max_radius_cells;
    const float* d_direction;
    const float* d_half_length;
    const float* d_sigma_x;
    const float* d_sigma_y;
    const float* d_rotation;
} pcr_hip_glyph;

/* Counters of the last scatter on an engine (diagnostics; exact). */
typedef struct pcr_hip_scatter_stats {
    uint64_t points_in;        /* points offered */
    uint64_t points_valid;     /* inside bounds and inside [own_row0, own_row1) */
    int32_t path;              /* 0 = direct global atomics, 1 = binned LDS tiles, 2 = moments + convolution */
    int32_t lds_tile_w, lds_tile_h, lds_apron, num_bins;
    int32_t scatter_chunk;     /* binned path: points per workgroup of the record-scatter pass (0 otherwise) */
    int32_t deferred_planes;   /* PCR_HIP_PLANE_* bits the scatter left in the bands it stored (pcr_hip_engine_defer_planes;
                                * the field was reserved_ and read 0) */
} pcr_hip_scatter_stats;

const char* pcr_hip_last_error(void);
int pcr_hip_abi_version(void);

/* ---- devices.  replaces: cuda_device_available/count/name/get_memory_info,
 *      include/pcr/core/types.h:156-219, and cudaSetDevice in src/engine/pipeline.cpp:133-160 */
int pcr_hip_device_count(int* count);
int pcr_hip_set_device(int device_id);
int pcr_hip_get_device(int* device_id);
int pcr_hip_device_name(int device_id, char* buf, size_t buf_len);
int pcr_hip_mem_info(size_t* free_bytes, size_t* total_bytes);
int pcr_hip_device_synchronize(void);

/* ---- streams / events.  replaces: the single cudaStream of src/engine/pipeline.cpp:198-213 */
int pcr_hip_stream_create(pcr_hip_stream* out);
int pcr_hip_stream_destroy(pcr_hip_stream s);
int pcr_hip_stream_synchronize(pcr_hip_stream s);
int pcr_hip_event_create(void** out);
int pcr_hip_event_destroy(void* ev);
int pcr_hip_event_record(void* ev, pcr_hip_stream s);
int pcr_hip_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* synchronizes on ev_stop */

/* ---- memory.  replaces: cudaMalloc/cudaMallocHost/cudaMemcpy* in src/core/point_cloud.cpp:55-73,
 *      382-512 (PointCloud::to / to_device_async) and src/core/grid.cpp device paths */
int pcr_hip_malloc(void** d_ptr, size_t bytes);
int pcr_hip_free(void* d_ptr);
int pcr_hip_host_alloc(void** h_ptr, size_t bytes);          /* pinned */
int pcr_hip_host_free(void* h_ptr);
int pcr_hip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, pcr_hip_stream s);  /* async when h_src is pinned */
int pcr_hip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, pcr_hip_stream s);
int pcr_hip_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, pcr_hip_stream s);
/* Device-to-device copy by a hand-written float4 kernel (16-byte aligned pointers and size; nontemporal != 0: loads and
 * stores that bypass the caches' allocation).  The yardstick bench.py reports as `measured_copy_GBps`: the streaming rate
 * this box really reaches, next to the 8 TB/s data-sheet peak (no reference counterpart: measurement only). */
int pcr_hip_copy_kernel(void* d_dst, const void* d_src, size_t bytes, int nontemporal, pcr_hip_stream s);
int pcr_hip_memset(void* d_ptr, int byte_value, size_t bytes, pcr_hip_stream s);

/* ---- arena.  replaces: pcr::MemoryPool (include/pcr/engine/memory_pool.h:18-50,
 *      src/engine/memory_pool.cu:24-59): bump allocator over one device allocation, 256-B aligned */
typedef struct pcr_hip_arena pcr_hip_arena;
int pcr_hip_arena_create(pcr_hip_arena** out, size_t bytes);
int pcr_hip_arena_destroy(pcr_hip_arena* a);
int pcr_hip_arena_alloc(pcr_hip_arena* a, size_t bytes, void** d_ptr);
int pcr_hip_arena_reset(pcr_hip_arena* a);
int pcr_hip_arena_stats(const pcr_hip_arena* a, size_t* capacity, size_t* used, size_t* high_water);
/* The scatter engine's own scratch (routing keys, records, moment planes) is one such arena per device, shared by
 * every engine on it, grow-only, borrowed exclusively for the duration of a scatter's enqueue (csrc/engine.hip):
 * capacity and high-water mark in bytes, number of borrows and of (re)allocations since process start. */
int pcr_hip_device_scratch_stats(int device, size_t* capacity, size_t* high_water, uint64_t* borrows, uint64_t* grows);

/* ---- state planes.  replaces: init_tile_state / merge_tile_state / finalize_tile,
 *      include/pcr/engine/grid_merge.h:22-41 (src/engine/grid_merge.cu:116-183), and the CPU
 *      finalize loop of src/engine/pipeline.cpp:1204-1286 (NaN fill, untouched tiles skipped) */
int pcr_hip_state_floats(int rtype, int* k);                                   /* reduction_registry.cpp:197-208 */
int pcr_hip_plane_fill(float* d_plane, float value, int64_t cells, pcr_hip_stream s);
int pcr_hip_state_init(int rtype, float* d_state, int64_t cells, pcr_hip_stream s);         /* K planes, stride = cells */
int pcr_hip_state_merge(int rtype, float* d_dst, const float* d_src, int64_t cells, pcr_hip_stream s);
/* merge one plane with the op of its PCR_HIP_PLANE_* kind (add / fmaxf / fminf): halo rows, multi-ingest merges */
int pcr_hip_plane_merge(uint32_t plane_kind, float* d_dst, const float* d_src, int64_t cells, pcr_hip_stream s);
/* out[row, col] for rows [own_row0, own_row1): finalize(rtype) of the planes where the cell's
 * reference tile is touched, NaN elsewhere.  d_out holds (own_row1-own_row0)*width floats.
 * d_tile_touched: tiles_x*tiles_y words (NULL = all touched). */
int pcr_hip_finalize(int rtype, const pcr_hip_grid* g, const pcr_hip_planes* planes,
                     const uint32_t* d_tile_touched, float* d_out, pcr_hip_stream s);

/* Same, for up to PCR_HIP_MAX_FINALIZE_OUTPUTS reductions that read ONE group's planes: each plane is
 * read once and every band written once (Sum + Count + Average of one channel: 2 plane reads, 3 band
 * writes instead of 4 + 3). */
#define PCR_HIP_MAX_FINALIZE_OUTPUTS 8
int pcr_hip_finalize_group(const pcr_hip_grid* g, const pcr_hip_planes* planes, const uint32_t* d_tile_touched,
                           int n_out, const int* rtypes, float* const* d_outs, pcr_hip_stream s);
/* Same, but a no-op when the word *d_bands_done is non-zero at the time the kernel runs (NULL: always runs): the bands
 * were already written by the scatter that defined the planes (pcr_hip_engine_finalize_with_scatter).  The launch itself is
 * still made; a caller that waits for the stream anyway and keeps the word in page-locked host memory (below) can read it
 * after the wait and not call at all, which is what the blocking Pipeline::finalize does. */
int pcr_hip_finalize_group_unless(const pcr_hip_grid* g, const pcr_hip_planes* planes, const uint32_t* d_tile_touched,
                                  int n_out, const int* rtypes, float* const* d_outs, const uint32_t* d_bands_done,
                                  pcr_hip_stream s);
/* The way back for planes a fused scatter left in its bands (pcr_hip_engine_defer_planes).  For every bit of plane_mask the
 * plane is stored over the whole state window from d_bands[slot] (slot 0 the Sum band, 1 Count, 2 Max, 3 Min; other slots are
 * not read) and the touched flags as they were when the scatter ran:
 *   Sum   = touched tile ? band : 0          Count = isnan(band) ? 0 : band
 *   Max   = isnan(band) ? -FLT_MAX : band    Min   = isnan(band) ? +FLT_MAX : band
 * A no-op when *d_bands_done reads 0 at the time the kernel runs (the scatter stored the planes itself), so it can be enqueued
 * without a host round trip.  The grid's owned rows must be its state window, width % 4 == 0, planes and bands 16-byte
 * aligned -- what the fused scatter required. */
int pcr_hip_planes_from_bands_if(const pcr_hip_grid* g, const pcr_hip_planes* planes, uint32_t plane_mask,
                                 const float* const* d_bands, const uint32_t* d_tile_touched, const uint32_t* d_bands_done,
                                 pcr_hip_stream s);

/* Union of another rank's touched-tile flags into this device's (row-block shards: a reference tile is touched if ANY rank saw
 * a point in it).  d_local[i] |= d_union[i] != 0, i < n; when that changed a flag, the n_words device words at d_bands_done
 * (may be NULL) are zeroed: bands that a scatter stored from the local flags alone are then stale and the finalize pass runs
 * (pcr_hip_finalize_group_unless).  Unchanged flags leave them alone -- the usual case on dense clouds. */
int pcr_hip_touched_union(uint32_t* d_local, const uint32_t* d_union, int32_t n, uint32_t* d_bands_done, int32_t n_words,
                          pcr_hip_stream s);
/* The same over a tiles_x x tiles_y flag grid for a device that owns rows of tile rows [own_tile_row0, own_tile_row1) only: a
 * flag that changes OUTSIDE that range is merged but leaves d_bands_done alone -- none of this device's bands depends on it
 * (non-tile-aligned row blocks: every other rank contributes tiles this one owns no row of). */
int pcr_hip_touched_union_owned(uint32_t* d_local, const uint32_t* d_union, int32_t tiles_x, int32_t tiles_y,
                                int32_t own_tile_row0, int32_t own_tile_row1, uint32_t* d_bands_done, int32_t n_words,
                                pcr_hip_stream s);

/* ---- scatter engine.  replaces: TileRouter::assign + sort + extract_batches
 *      (include/pcr/engine/tile_router_kernels.h:15-52, src/engine/tile_router.cpp:51-366),
 *      Accumulator::accumulate (include/pcr/engine/accumulator_kernels.h:13-23,
 *      src/engine/accumulator.cpp:33-59) and accumulate_glyph
 *      (include/pcr/engine/glyph_kernels.h:31-42), fused: no sort, no materialised indices. */
typedef struct pcr_hip_engine pcr_hip_engine;
/* scratch_bytes = 0: the engine grows its scratch arena on demand (the arena is shared by all engines of a device).
 * Test-only environment knobs, read here: PCR_HIP_DEBUG_MAX_BINS=<n> lowers the number of LDS tiles one binning pass
 * may count (8064) so that the large-grid paths (two-level sort, row bands) are reached on small grids;
 * PCR_HIP_DEBUG_TWO_LEVEL=0 forces the row-band sweep where the two-level sort would apply
 * (the passes on 16-byte glyph records count up to 16384 tiles: the knob applies to them as it stands).
 * PCR_HIP_TUNE_CONV=1|2 forces the vector-ALU | matrix-core column pass of the moment path whatever the radius (tests reach
 * both kernels on small shapes), PCR_HIP_CONV_WAVES=4|8 the workgroup shape of the matrix-core pass, PCR_HIP_CELL_TILE_H=<rows>
 * the height of the Gaussian cell tiles (read at scatter time): shapes only, results do not change.  PCR_HIP_RCCL=<path> names
 * the RCCL library pcr_hip_comm_* loads (default: the copy the process already has, else the one beside libamdhip64). */
int pcr_hip_engine_create(pcr_hip_engine** out, const pcr_hip_grid* g, size_t scratch_bytes, pcr_hip_stream s);
int pcr_hip_engine_destroy(pcr_hip_engine* e);
/* 0 = auto, 1 = force direct global atomics, 2 = force binned LDS tiles (INVALID_ARGUMENT if the grid cannot
 * be binned), 3 = force the separable moment + convolution path for Gaussians (other glyphs: as auto) */
int pcr_hip_engine_set_path(pcr_hip_engine* e, int path);
/* State of the planes handed to the NEXT pcr_hip_scatter_point / _glyph only (cleared by it).  Wrong hint = wrong results.
 *   0  they hold earlier contributions: the merge read-modify-writes (the default);
 *   1  every cell holds its identity value (just filled by pcr_hip_plane_fill / pcr_hip_state_init, nothing accumulated
 *      or loaded since): the Point tile-merge stores instead of read-modify-writing (saves one read of the planes);
 *   2  they are UNDEFINED (never filled): the scatter itself leaves every cell of the state window defined -- the binned
 *      Point path by storing every cell of every LDS tile, identity included (no pass of its own; a bin the scan had to
 *      split, or a window swept in several bands / two sort levels, falls back to filling first), the moment path by
 *      letting its row pass store instead of accumulate (one window over the whole state window; else it fills first),
 *      every other path by filling the planes with identity values before it accumulates (timed as `k_state_init`).
 * The reference initialises tile state inside ingest, on first acquire (src/engine/tile_manager.cpp:272-320,
 * src/engine/pipeline.cpp:688-691): with 2 this build's state initialisation is inside the ingest as well. */
int pcr_hip_engine_planes_fresh(pcr_hip_engine* e, int fresh);
/* Finalize fused into the scatter that defines the planes -- for the NEXT pcr_hip_scatter_point only (cleared by it).
 * When that scatter runs with planes_fresh = 2 on the binned path and its tile pass stores every cell of the state
 * window itself, the same pass also stores the finished bands (finalize(rtype) of the cell where its reference tile is
 * touched BY THIS SCATTER'S points, NaN elsewhere) from the LDS tile it has in hand: the planes are not read again
 * (Pipeline::finalize after a pipeline's only ingest: src/engine/pipeline.cpp:1154-1286 reads every tile's state back).
 * d_outs[i] holds own_rows * width floats, 16-byte aligned; the engine's owned rows must be its whole state window.
 * *d_bands_done is written by the scatter, with one 4-byte store from the device: 1 when every band cell was stored, 0
 * when the pass could not (a bin the scan had to split).  The word lives in any memory the device can address: device
 * memory, or page-locked host memory from pcr_hip_host_alloc (mapped into the device's address space under the same
 * pointer), which the host may read once the stream has been synchronised.  pcr_hip_engine_finalize_taken: 1 when the last pcr_hip_scatter_point launched the
 * fused form at all (else *d_bands_done was not written and the bands are untouched).  The bands stay valid only while
 * nothing else changes the planes or the touched flags: the caller decides (pcr_hip_finalize_group_unless). */
int pcr_hip_engine_finalize_with_scatter(pcr_hip_engine* e, int n_out, const int* rtypes, float* const* d_outs,
                                         uint32_t* d_bands_done);
int pcr_hip_engine_finalize_taken(const pcr_hip_engine* e);
/* Planes the NEXT pcr_hip_scatter_point may leave UNSTORED (PCR_HIP_PLANE_* bits; cleared by that scatter; send it after
 * pcr_hip_engine_finalize_with_scatter, which resets it).  For the Point glyph a plane whose own reduction (Sum, Count, Max,
 * Min) is one of the bands the fused tile pass stores is a bit-exact function of that band and the touched flags, so the pass
 * can skip the plane's store and a caller that only finalizes never pays for it.  The engine takes a bit only when the
 * launch is the fused one and the plane's own reduction is among the bands given; every other bit is dropped and the plane
 * stored as always.  pcr_hip_engine_planes_deferred: the bits the last pcr_hip_scatter_point took.  They hold only where
 * *d_bands_done reads 1 once the scatter has run -- where it reads 0 every plane was stored.  While a plane is deferred its
 * memory is UNDEFINED and its band must not be written: pcr_hip_planes_from_bands_if puts it back.  A caller that never sends
 * the hint gets every store. */
int pcr_hip_engine_defer_planes(pcr_hip_engine* e, uint32_t plane_mask);
int pcr_hip_engine_planes_deferred(const pcr_hip_engine* e);
int pcr_hip_engine_stats(const pcr_hip_engine* e, pcr_hip_scatter_stats* out);
/* device array of tiles_x*tiles_y words, non-zero where a valid point's centre cell fell */
int pcr_hip_engine_tile_touched(pcr_hip_engine* e, uint32_t** d_tile_touched, int32_t* tiles_x, int32_t* tiles_y);

/* ---- point filter.  replaces: filter_points (include/pcr/engine/filter.h:65-74; CPU src/engine/filter.cpp:34-206,
 *      CUDA kernel_evaluate_predicates src/engine/filter_kernels.cu:22-64): AND of per-channel predicates on
 *      Float32 channels.  Produces a byte mask (1 = keep) instead of a compacted index list; the engine applies
 *      the mask inside its routing kernels, so a filtered ingest costs one extra byte per point. */
#define PCR_HIP_MAX_FILTER_PREDICATES 16
#define PCR_HIP_MAX_FILTER_SET 16          /* the reference's device limit (src/engine/filter_kernels.cu:15) */
enum {                                      /* pcr::CompareOp numbering (include/pcr/engine/filter.h:20-29) */
    PCR_HIP_CMP_EQUAL = 0, PCR_HIP_CMP_NOT_EQUAL = 1, PCR_HIP_CMP_LESS = 2, PCR_HIP_CMP_LESS_EQUAL = 3,
    PCR_HIP_CMP_GREATER = 4, PCR_HIP_CMP_GREATER_EQUAL = 5, PCR_HIP_CMP_IN_SET = 6, PCR_HIP_CMP_NOT_IN_SET = 7
};
typedef struct pcr_hip_predicate {
    const float* d_channel;
    int32_t op;
    float value;
    int32_t set_size;
    float set[PCR_HIP_MAX_FILTER_SET];
} pcr_hip_predicate;
/* d_mask[i] = all predicates hold for point i; *d_pass_count (optional, device u64, zeroed by the call) = survivors */
int pcr_hip_filter_mask(const pcr_hip_predicate* preds, int n_pred, uint64_t n, uint8_t* d_mask,
                        unsigned long long* d_pass_count, pcr_hip_stream s);
/* Points with d_mask[i] == 0 are ignored by every following scatter on this engine; NULL clears it. */
int pcr_hip_engine_set_point_mask(pcr_hip_engine* e, const uint8_t* d_mask);

/* ---- per-reduction point filters (ReductionSpec::filter; no reference counterpart).  Several reductions of one ingest each
 *      see their own subset of the points: ONE sweep evaluates a table of DISTINCT predicates and stores one byte mask per
 *      filter CLASS, each in the layout pcr_hip_engine_set_point_mask takes.
 *   preds[0 .. n_pred)        the distinct predicates, at most PCR_HIP_MAX_CLASS_PREDICATES (they travel as kernel arguments:
 *                             32 x 80 B fit the 4 KB a kernel may take; a longer table would have to live in device memory)
 *   class_predicates[j]       bit k set: class j ANDs preds[k]; 0: the class keeps every point; 1..PCR_HIP_MAX_FILTER_CLASSES
 *                             classes.  By convention class 0 is PipelineConfig::filter alone when one is asked for: the
 *                             pipelines' one caller (detail::sweep_filter_classes) runs every filtered ingest through this
 *                             sweep, a pipeline with PipelineConfig::filter and no spec filter as the table of one class.
 *   d_masks + j * mask_stride class j's mask, n bytes (1 = keep); mask_stride >= n
 *   d_counts                  optional, n_classes device u64 zeroed by the call: survivors per class
 *      A channel is loaded once per point however many classes read it and a predicate evaluated once; with 16-byte aligned
 *      channels and 4-byte aligned masks (base and stride) the sweep loads 16 bytes per lane and channel and stores the four
 *      mask bytes of a lane packed.  Semantics are pcr_hip_filter_mask's: a NaN fails every op but NotEqual and NotInSet.
 *      Argument errors (null tables, 0 or more than 8 classes, a class naming a predicate outside the table) are answered on
 *      the host with PCR_HIP_INVALID_ARGUMENT before anything touches a device. */
#define PCR_HIP_MAX_FILTER_CLASSES 8
#define PCR_HIP_MAX_CLASS_PREDICATES 32
int pcr_hip_filter_classes(const pcr_hip_predicate* preds, int n_pred, const uint32_t* class_predicates, int n_classes, uint64_t n,
                           uint8_t* d_masks, uint64_t mask_stride, unsigned long long* d_counts, pcr_hip_stream s);
/* Sets the engine's touched-tile flags from the points its current point mask keeps -- exactly the flags a
 * pcr_hip_scatter_point of the same points would set (bounds, owned rows, the one-tile case, division as in world_to_cell)
 * -- on the engine's stream, and writes no plane.  For an ingest none of whose groups is unfiltered: the touched flags of a
 * pipeline come from PipelineConfig::filter's survivors, never from a reduction's own filter. */
int pcr_hip_engine_touch(pcr_hip_engine* e, const double* d_x, const double* d_y, uint64_t n);

/* ---- multi-GPU routing of an unpartitioned cloud.  No reference counterpart: the reference is single-device and
 *      its 1 B-point protocol feeds one pipeline (scripts/benchmarks/benchmark_billion_points.py:221-345).  With the
 *      grid row-block sharded over GPUs, a rank groups the points it was handed by OWNER (the part whose row range
 *      holds the point's centre row: GridConfig::world_to_cell, src/core/grid_config.cpp:24-43, exactly as the
 *      scatter kernels evaluate it), the groups travel point-to-point (RCCL all-to-all, pcr/distributed.py), and
 *      every rank ingests only points it owns.
 *   route_count:   d_dest[i] = owning part (0xFF: outside the grid / masked out / owned by nobody);
 *                  d_counts[p] (device u64, zeroed by the call) = points owned by part p.
 *                  row_splits: HOST array of nparts+1 ascending rows, part p owns [row_splits[p], row_splits[p+1]).
 *   route_scatter: regroups up to 8 arrays of 4- or 8-byte elements by owner; d_cursors[p] (device u64) holds the
 *                  first output slot of part p on entry (exclusive prefix sums of the counts) and is advanced.
 *                  Order inside a part is unspecified. */
#define PCR_HIP_MAX_ROUTE_PARTS 64
#define PCR_HIP_MAX_ROUTE_ARRAYS 8
int pcr_hip_route_count(const pcr_hip_grid* g, const int32_t* row_splits, int nparts,
                        const double* d_x, const double* d_y, const uint8_t* d_mask, uint64_t n,
                        uint8_t* d_dest, unsigned long long* d_counts, pcr_hip_stream s);
int pcr_hip_route_scatter(const uint8_t* d_dest, uint64_t n, int nparts, unsigned long long* d_cursors,
                          int narrays, const void* const* d_src, void* const* d_dst, const int32_t* elem_bytes,
                          pcr_hip_stream s);
/* max |d_values[i]| over the finite entries (0 for n == 0), synchronizes the stream.  Sizes the halo check of a
 * row-block shard whose Line glyph has a per-point half_length channel (its y reach is not capped by
 * max_radius_cells: glyph_kernels.cu:228-234). */
int pcr_hip_absmax_f32(const float* d_values, uint64_t n, float* h_result, pcr_hip_stream s);
/* The same over the points a filter mask keeps (d_mask may be NULL), with the 4-byte device word the reduction needs
 * supplied by the caller (NULL: allocated and freed inside, which synchronizes the whole device). */
int pcr_hip_absmax_f32_masked(const float* d_values, const uint8_t* d_mask, uint64_t n, uint32_t* d_scratch_word,
                              float* h_result, pcr_hip_stream s);
/* max(+v) and max(-v) over the finite entries the mask keeps (each >= 0; d_scratch_2words: 8 bytes of device memory).
 * The reference caps a Line's y half-extent with std::min(hy, cap), hy = half_length / cell_size_y (glyph_kernels.cu:228-234):
 * only the sign of half_length that makes hy POSITIVE is capped, so a shard's halo check needs the two sides apart. */
int pcr_hip_signed_max_f32_masked(const float* d_values, const uint8_t* d_mask, uint64_t n, uint32_t* d_scratch_2words,
                                  float* h_max_pos, float* h_max_neg, pcr_hip_stream s);

/* ---- multi-device: the exchange step of row-block shards, over RCCL / xGMI.  New work: the reference is single-device
 *      (cuda_device_id, include/pcr/engine/pipeline.h:68); SURVEY section 8b asks for these entry points, 8e fixes their
 *      shape.  One process per GPU; rank r owns rows [own_row0, own_row1) and keeps `halo` apron rows on each side inside
 *      its state window [state_row0, state_row0 + state_rows).
 *        halo_reduce        apron rows -> the neighbour that owns them (ncclSend/ncclRecv to rank +- 1 in one group),
 *                           merged there with the plane's op (add for SUM / WGT, fmaxf / fminf for MAX / MIN)
 *        allreduce_max_u32  the touched-tile flags (one word per reference tile)
 *      Both are enqueued on the caller's stream.  RCCL is loaded on first use (librccl.so.1); without it the calls
 *      return PCR_HIP_NOT_IMPLEMENTED and pcr_hip_comm_available() is 0.  Bootstrap: rank 0 makes a 128-byte id, the
 *      host carries it to the other ranks (MPI, a file, torch.distributed, ...), every rank calls _create. */
#define PCR_HIP_COMM_ID_BYTES 128
typedef struct pcr_hip_comm pcr_hip_comm;
typedef struct pcr_hip_halo_plane {
    float* d_plane;            /* state_rows x width floats */
    uint32_t kind;             /* PCR_HIP_PLANE_SUM / _WGT / _MAX / _MIN */
    uint32_t reserved_;
} pcr_hip_halo_plane;
int pcr_hip_comm_available(void);
int pcr_hip_comm_unique_id(uint8_t* id128);
int pcr_hip_comm_create(pcr_hip_comm** out, const uint8_t* id128, int rank, int world, int device);
int pcr_hip_comm_destroy(pcr_hip_comm* c);
int pcr_hip_comm_rank(const pcr_hip_comm* c, int* rank, int* world);
/* halo_reduce cannot hang on arguments that disagree between the ranks: every call first ALL-GATHERS what each rank brings
 * (one pcr_hip_halo_geom, posted whatever this rank's own arguments were; costs one small collective + a stream sync),
 * every rank judges the gathered records with the same pure function (pcr_hip_comm_halo_plan), and either all of them post
 * their sends and receives -- a receive sized from what its sender says it holds -- or all of them return
 * PCR_HIP_INVALID_ARGUMENT with the same message (a block shorter than a neighbour's apron, blocks that are not contiguous,
 * a rank that owns no rows, different widths / halos / planes, a rank with invalid arguments).  At most 8 planes per call. */
typedef struct pcr_hip_halo_geom {
    int32_t width, state_row0, state_rows, own_row0, own_row1, halo, nplanes;
    int32_t kinds;             /* plane kinds, 4 bits each, plane 0 in the low bits */
    int32_t valid;             /* 0: this rank's own arguments were unusable -- everyone refuses */
    int32_t reserved_;
} pcr_hip_halo_geom;
int pcr_hip_comm_halo_reduce(pcr_hip_comm* c, const pcr_hip_halo_plane* planes, int nplanes, int width,
                             int state_row0, int state_rows, int own_row0, int own_row1, int halo, pcr_hip_stream s);
/* The verdict on `world` gathered records, and rank's message sizes in rows (0: no message).  Pure host code: no
 * communicator, no device -- what the CPU tests drive. */
int pcr_hip_comm_halo_plan(const pcr_hip_halo_geom* all, int world, int rank, int* send_up_rows, int* send_dn_rows,
                           int* recv_up_rows, int* recv_dn_rows);
/* MAX over the ranks of one host integer (collective; synchronizes the stream): what a sharded ingest agrees on before
 * anything is accumulated, e.g. the Line reach of this round's clouds, so that every rank refuses together. */
int pcr_hip_comm_agree_max_i32(pcr_hip_comm* c, int32_t* h_inout, pcr_hip_stream s);
int pcr_hip_comm_allreduce_max_u32(pcr_hip_comm* c, uint32_t* d_words, int count, pcr_hip_stream s);
int pcr_hip_comm_allreduce_sum_f64(pcr_hip_comm* c, double* d_values, int count, pcr_hip_stream s);
int pcr_hip_comm_stats(const pcr_hip_comm* c, uint64_t* halo_reduces, uint64_t* bytes_sent);
/* Variable-size transfers (round 5), with the halo reduce's discipline: what every rank brings is all-gathered first (one
 * pcr_hip_xfer_geom each, posted whatever the rank's own arguments were), every rank passes the same verdict on the gathered
 * records (pcr_hip_comm_xfer_plan, pure host code), and either all post their sends and receives -- a receive sized from what
 * its sender announced -- or all return PCR_HIP_INVALID_ARGUMENT with the same message.  Up to 8 arrays travel in ONE group with
 * the same element counts (a cloud's x, y and channels; a result's bands); array a has elem_bytes[a]-byte elements (1..16).
 *   alltoallv       SURVEY section 8e "device-side partition + peer copy": d_send[a] holds this rank's elements grouped by
 *                   destination rank (h_send_counts[p] elements for rank p, in rank order: pcr_hip_route_scatter's output);
 *                   d_recv[a] receives the groups of all ranks in rank order; h_recv_counts[p] (optional) = elements from p.
 *                   recv_capacity = elements d_recv[a] can hold: a rank that would overflow makes every rank refuse.
 *   alltoall_counts the counts alone (every rank's h_send_counts row to every rank): sizes the receive buffers beforehand.
 *   gatherv         every rank's send_count elements per array to `root`, landing there in rank order (the row strips of a
 *                   sharded result -> one grid, src/engine/pipeline.cpp:1175-1186, 1351-1361 write ONE file).
 * A rank's own group is a device-to-device copy; a world of one needs no RCCL at all.  All on the caller's stream. */
#define PCR_HIP_MAX_XFER_ARRAYS 8
typedef struct pcr_hip_xfer_geom {
    int32_t narrays;
    int32_t elem_bytes[PCR_HIP_MAX_XFER_ARRAYS];
    int32_t root;              /* gatherv: the receiving rank; alltoallv: -1 */
    int32_t valid;             /* 0: this rank's own arguments were unusable -- everyone refuses */
    int32_t reserved_;
    uint64_t recv_capacity;    /* elements per array this rank can take */
    uint64_t send_counts[PCR_HIP_MAX_ROUTE_PARTS];   /* elements per array this rank sends to rank p */
} pcr_hip_xfer_geom;
int pcr_hip_comm_alltoall_counts(pcr_hip_comm* c, const uint64_t* h_send_counts, uint64_t* h_recv_counts, pcr_hip_stream s);
int pcr_hip_comm_alltoallv(pcr_hip_comm* c, int narrays, const void* const* d_send, void* const* d_recv, const int32_t* elem_bytes,
                           const uint64_t* h_send_counts, uint64_t recv_capacity, uint64_t* h_recv_counts, pcr_hip_stream s);
int pcr_hip_comm_gatherv(pcr_hip_comm* c, int narrays, const void* const* d_send, void* const* d_recv, const int32_t* elem_bytes,
                         uint64_t send_count, uint64_t recv_capacity, uint64_t* h_recv_counts, int root, pcr_hip_stream s);
/* send_offsets / recv_offsets: world + 1 entries (the last = totals); recv_counts: world entries. */
int pcr_hip_comm_xfer_plan(const pcr_hip_xfer_geom* all, int world, int rank, uint64_t* send_offsets, uint64_t* recv_counts,
                           uint64_t* recv_offsets);

/* Per-kernel timing with HIP events on the engine's stream (for roofline reporting).
 * While enabled every kernel the engine launches is bracketed by two events; _read drains the
 * events (synchronizes) and returns, per kernel name, launches and summed milliseconds. */
typedef struct pcr_hip_kernel_time {
    char name[48];
    uint32_t launches;
    double total_ms;
} pcr_hip_kernel_time;
int pcr_hip_engine_profile_enable(pcr_hip_engine* e, int on);
/* Every pair of events costs the stream ~4 us of serialisation (measured: 52 us on a 0.69 ms step with 7 kernels).
 * kernel_name != NULL / "": only launches timed under that name are bracketed (a roofline needs one kernel, and the
 * step around it should run as it does in production); NULL or "": all of them. */
int pcr_hip_engine_profile_only(pcr_hip_engine* e, const char* kernel_name);
int pcr_hip_engine_profile_read(pcr_hip_engine* e, pcr_hip_kernel_time* out, int capacity, int* count, int reset);

/* Point glyph: every valid point folds `value` into the planes named by plane_mask at its cell.
 * d_value may be NULL only when plane_mask == PCR_HIP_PLANE_WGT. */
int pcr_hip_scatter_point(pcr_hip_engine* e, uint32_t plane_mask, const pcr_hip_planes* planes,
                          const double* d_x, const double* d_y, const float* d_value, uint64_t n);
/* Line / Gaussian glyph: planes SUM (+= v*w) and/or WGT (+= w) only. */
int pcr_hip_scatter_glyph(pcr_hip_engine* e, const pcr_hip_glyph* glyph, uint32_t plane_mask,
                          const pcr_hip_planes* planes,
                          const double* d_x, const double* d_y, const float* d_value, uint64_t n);

/* ---- MostRecent: per cell, the value of the point with the greatest key (timestamp).  Point glyph only.
 *      replaces: MostRecentOp / combine_timestamped (include/pcr/ops/builtin_ops.h:106-124), which the reference declares but
 *      never registers, and its racy kernel_accumulate_most_recent (src/engine/accumulator_kernels.cu:136-167).
 *   On the device a group's state is ONE plane of packed 64-bit words in grid layout (8 bytes per cell):
 *      ord(f)     = bits(f) ^ (sign(f) ? 0xFFFFFFFF : 0x80000000)        (monotone float -> unsigned)
 *      word(t, v) = (uint64(ord(t + 0.0f)) << 32) | ord(v)
 *   A point is ACCEPTED when it is inside the bounds and the owned rows, the mask keeps it, and its key t satisfies t == t and
 *   t > -FLT_MAX.  A cell holds the MAXIMUM word of its accepted points, 0 when it has none (every accepted word is
 *   > 0x0080000000000000: a memset defines the plane).  Among equal keys the greater value by ord() wins; a NaN value is
 *   copied like any other.  The fold is associative, commutative and idempotent: every path, split and order gives the same
 *   bits.  At the boundary (checkpoints, `.pcrt` files, host copies) the state is the reference's layout, two float planes:
 *   plane 0 the value, plane 1 the key, an empty cell {NaN 0x7FC00000, -FLT_MAX} (pack_state<MostRecentOp>,
 *   builtin_ops.h:178-183); pcr_hip_state_init / _merge of type 8 work on that layout (d_state = 2 planes, stride = cells).
 *      select_pack      float planes -> words (a NaN or <= -FLT_MAX key means empty)
 *      select_unpack    words -> float planes
 *      select_merge     d_dst[i] = max(d_dst[i], d_src[i]), 64-bit unsigned
 *      scatter_select   the scatter; honours pcr_hip_engine_set_path (1 direct: one 64-bit global atomic max per accepted
 *                       point; 2 binned: 8-byte index records, one 64-bit LDS atomic max per record, tile merge; 0 / 3 auto),
 *                       pcr_hip_engine_planes_fresh (0 / 1 / 2, with "identity" = 0), the point mask, the owned rows, the
 *                       touched flags, pcr_hip_engine_stats and the profile timers, like pcr_hip_scatter_point
 *      finalize_select  out = value where the word is non-zero and the cell's reference tile is touched, NaN elsewhere;
 *                       rows [own_row0, own_row1) as pcr_hip_finalize */
int pcr_hip_select_pack(const float* d_value, const float* d_key, uint64_t* d_packed, int64_t cells, pcr_hip_stream s);
int pcr_hip_select_unpack(const uint64_t* d_packed, float* d_value, float* d_key, int64_t cells, pcr_hip_stream s);
int pcr_hip_select_merge(uint64_t* d_dst, const uint64_t* d_src, int64_t cells, pcr_hip_stream s);
int pcr_hip_scatter_select(pcr_hip_engine* e, uint64_t* d_packed, const double* d_x, const double* d_y,
                           const float* d_value, const float* d_key, uint64_t n);
int pcr_hip_finalize_select(const pcr_hip_grid* g, const uint64_t* d_packed, const uint32_t* d_tile_touched, float* d_out,
                            pcr_hip_stream s);

/* ---- coordinate reprojection.  No reference counterpart: PipelineConfig::target_crs / auto_reproject are declared there
 *      (include/pcr/engine/pipeline.h:55-56) and src/engine/reprojection.cpp is a TODO.  No PROJ: a fixed set of EPSG codes
 *      resolves to a descriptor, and every transform goes source -> geographic -> destination.
 *        geographic   4326 (WGS 84), 4269 (NAD83), 4258 (ETRS89): x = longitude, y = latitude, degrees
 *        web mercator 3857 (spherical formulas on a = 6378137)
 *        UTM          32601-32660 / 32701-32760 (WGS 84, north / south), 26901-26923 (NAD83), 25828-25838 (ETRS89):
 *                     Krueger's series to n^6 (Karney 2011), k0 0.9996, FE 500 000, FN 0 / 10 000 000
 *      WGS 84, NAD83 and ETRS89 are one datum here (no datum shift: PROJ's "ballpark" transformation without grids).
 *      A point outside the domain becomes NaN on both axes: a non-finite coordinate on either axis, |latitude| > 90, the
 *      poles for 3857, and for UTM, in both directions, |eta'| > 1 with eta' = atanh(cos(conformal latitude) sin(lon - lon0))
 *      -- about 50 degrees from the central meridian on the equator, any |lon - lon0| < 90 near the poles (the poles
 *      themselves at any longitude); the inverse also refuses northings beyond the pole.  Inside, UTM is within 1e-6 m
 *      (forward) and 1e-10 degrees (inverse) of the exact Gauss-Krueger map.  Two descriptors of the same code
 *      copy the coordinates bit for bit; two geographic ones copy them too (NaN where |latitude| > 90 or non-finite).  out_x / out_y are either x / y themselves (in place) or do not overlap them. */
enum { PCR_HIP_CRS_GEOGRAPHIC = 1, PCR_HIP_CRS_WEB_MERCATOR = 2, PCR_HIP_CRS_TRANSVERSE_MERCATOR = 3 };
typedef struct pcr_hip_crs_desc {
    int32_t epsg;
    int32_t kind;                    /* PCR_HIP_CRS_* */
    double a, f;                     /* ellipsoid (web mercator: the sphere's radius a, f = 0) */
    double lon0;                     /* central meridian, degrees */
    double k0, fe, fn;               /* scale on the central meridian, false easting / northing (metres) */
    double e;                        /* first eccentricity */
    double ka;                       /* k0 * rectifying radius */
    double alpha[6], beta[6];        /* Krueger series: forward, inverse */
    double delta[6];                 /* conformal -> geodetic latitude series */
} pcr_hip_crs_desc;
/* PCR_HIP_NOT_IMPLEMENTED (with the code in pcr_hip_last_error) for a code outside the list above. */
int pcr_hip_crs_from_epsg(int epsg, pcr_hip_crs_desc* out);
/* n points on the device, enqueued on s. */
int pcr_hip_transform_xy(const pcr_hip_crs_desc* src, const pcr_hip_crs_desc* dst, const double* d_x, const double* d_y,
                         double* d_out_x, double* d_out_y, uint64_t n, pcr_hip_stream s);
/* The same on host arrays, in the calling thread (pure, thread-safe: the host engine calls it from its OpenMP loop). */
int pcr_hip_transform_xy_host(const pcr_hip_crs_desc* src, const pcr_hip_crs_desc* dst, const double* h_x, const double* h_y,
                              double* h_out_x, double* h_out_y, uint64_t n);

/* ---- overview pyramid of one band (GeoTIFF overviews; pcr/io/grid_io.h: build_overviews).  Level k (k >= 1) is made from
 *      level k-1 (level 0 = src) and is ceil(w/2) x ceil(h/2) cells; cell (r, c) looks at (2r, 2c), (2r, 2c+1), (2r+1, 2c),
 *      (2r+1, 2c+1); a cell outside the source or a NaN cell is invalid.  mode 0 "average": the invalid cells contribute
 *      +0.0f, s = ((a + b) + c) + d in binary32, result s / n over the n valid cells (a true division), NaN when n == 0;
 *      every NaN made here (Inf + -Inf included) is 0x7FC00000.  mode 1 "nearest": cell (2r, 2c), copied bit for bit.
 *      src: `height` rows of `width` floats, `src_stride` floats apart (any 4-byte alignment; rows that start on 16 bytes
 *      take the 16-byte loads).  dst: a HOST array of `levels` device pointers, dense planes of the levels' sizes.  The
 *      source is read once per six levels; everything is enqueued on s, nothing is allocated or synchronised. */
int pcr_hip_downsample2(const float* src, int width, int height, int64_t src_stride, float* const* dst, int levels, int mode,
                        pcr_hip_stream s);

/* ---- no-data cells of one band filled from their neighbours (pcr/core/fill_nodata.h: fill_nodata), out of place.
 *      A cell of src that is not NaN is copied bit for bit.  For a NaN cell at (r, c) the window offsets are visited in
 *      row-major order, dr = -radius..radius and inside it dc = -radius..radius; an offset is skipped when
 *      d2 = dr*dr + dc*dc is 0 or greater than radius*radius, when (r+dr, c+dc) is outside the image, or when the source
 *      cell there is NaN.  Every other offset contributes with w = 1.0f / (float)d2 (correctly rounded binary32) to two
 *      binary64 sums that start at +0.0: s += (double)w * (double)v; t += (double)w -- the order of the additions is part
 *      of the contract.  t == 0: the source NaN, bit for bit.  Otherwise (float)(s / t), a true binary64 division rounded
 *      to nearest even; a NaN result (Inf + -Inf among the neighbours) is 0x7FC00000; +-Inf and denormals are values.
 *      Every read is of src: filling never chains, a hole wider than 2 * radius keeps a NaN core.
 *      src, dst: `height` rows of `width` floats, `src_stride` / `dst_stride` floats apart (any 4-byte alignment; rows of
 *      both that start on 16 bytes take the 16-byte accesses); they must not overlap.  1 <= radius <= 32.  Argument errors
 *      are reported before any HIP call.  Enqueued on s; nothing is allocated or synchronised. */
int pcr_hip_fill_nodata(const float* src, float* dst, int width, int height, int64_t src_stride, int64_t dst_stride, int radius,
                        pcr_hip_stream s);

/* ---- ground filter: a progressive morphological filter on one band (pcr/core/ground_filter.h: ground_filter; Zhang et al.
 *      2003), out of place, NaN = no data.
 *        erode(A, R)(r, c) is the minimum of the non-NaN cells of A in rows r-R..r+R and columns c-R..c+R clipped to the
 *        image, NaN when there is none; dilate is the same with the maximum.  NaN cells are ignored, never propagated (minNum
 *        / maxNum).  A0 = src.  For k = 1..levels: Ok = dilate(erode(Ak-1, radii[k]), radii[k]); a cell with non-NaN src
 *        becomes non-ground when Ak-1(c) - Ok(c) > thresholds[k] (one binary32 subtraction rounded to nearest, a NaN
 *        difference compares false); then Ak = Ok.  Once non-ground, a cell stays non-ground.
 *        dst(c) = src(c) bit for bit where src(c) is not NaN and the cell never became non-ground, 0x7FC00000 everywhere
 *        else.  +-Inf and denormals are values.  The result does not depend on the evaluation order.
 *      1 <= levels <= 64; 1 <= radii[0] < radii[1] < ... <= 64; every threshold finite and >= 0.  radii and thresholds are
 *      HOST arrays.  src, dst: `height` rows of `width` floats, `src_stride` / `dst_stride` floats apart (any 4-byte
 *      alignment; rows that start on 16 bytes take the 16-byte accesses).  d_work: device memory of at least
 *      pcr_hip_ground_filter_work_bytes(width, height) bytes (three planes; answered without a device).  dst and the
 *      workspace must not overlap src (nor each other).  Argument errors are reported before any HIP call.  Everything is
 *      enqueued on s; nothing is allocated or synchronised. */
int pcr_hip_ground_filter_work_bytes(int width, int height, size_t* bytes);
int pcr_hip_ground_filter(const float* src, float* dst, int width, int height, int64_t src_stride, int64_t dst_stride, int levels,
                          const int* radii, const float* thresholds, void* d_work, size_t work_bytes, pcr_hip_stream s);
/*      Height above ground: dst(c) = top(c) - ground(c), one binary32 subtraction; 0x7FC00000 when an operand or the result
 *      is NaN.  Strides in floats, any 4-byte alignment; dst may be top or ground.  Enqueued on s. */
int pcr_hip_band_difference(const float* top, const float* ground, float* dst, int width, int height, int64_t top_stride,
                            int64_t ground_stride, int64_t dst_stride, pcr_hip_stream s);

/* ---- terrain bands of one band (pcr/core/terrain.h: terrain; what gdaldem derives from a DEM), every product asked for in
 *      one launch that reads src once.  a b c / d e f / g h i is the 3 x 3 window around cell e, row a b c being image row
 *      r - 1.  NaN is "no data"; every NaN stored is 0x7FC00000.  A neighbour outside the image or NaN is missing: with
 *      edges = 0 (gdaldem's default) a cell with any missing neighbour is NaN, with edges = 1 (gdaldem -compute_edges) a
 *      missing neighbour takes e's value; e NaN gives NaN in both.
 *        Gradients (Horn), binary64, additions in this order, never fused:  GX = ((c + 2f) + i) - ((a + 2d) + g),
 *        GY = ((a + 2b) + c) - ((g + 2h) + i), p = GX * kx with kx = z_factor / (8.0 * cell_size_x), q = GY * ky with
 *        ky = z_factor / (-8.0 * cell_size_y), s2 = p*p + q*q.  The cell sizes are signed: on a north-up grid
 *        (cell_size_y < 0) p is dz/dEast and q is dz/dNorth.
 *        SLOPE_DEGREES  atan_deg((float)sqrt(s2));  SLOPE_PERCENT  (float)(100.0 * sqrt(s2))
 *        ASPECT         compass bearing of the downslope direction (-p, -q) in [0, 360), -1.0f where p == 0 and q == 0:
 *                       t = atan_deg((float)(|p| / |q|)); q <= 0: p > 0 ? 360 - t : t; q > 0: p > 0 ? 180 + t : 180 - t, in
 *                       binary32; 360 becomes 0
 *        HILLSHADE      L = (sin_alt - (p * ls + q * lc)) / sqrt(1.0 + s2); 1.0f when L <= 0, else (float)(1.0 + 254.0 * L);
 *                       ls = cos_alt * sin_az, lc = cos_alt * cos_az (pcr::terrain_light: the device evaluates no sine)
 *        TRI            (float)((|a-e| + |b-e| + |c-e| + |d-e| + |f-e| + |g-e| + |h-e| + |i-e|) / 8.0), binary64, left to right
 *        TPI            (float)(e - (a + b + c + d + f + g + h + i) / 8.0), binary64, left to right
 *        ROUGHNESS      max9 - min9, one binary32 subtraction; the maximum starts at a and takes b .. i in turn when greater,
 *                       the minimum when less
 *        sqrt and / are correctly rounded; atan_deg is Cephes' atanf (reduction at tan pi/8 and tan 3pi/8, 4-term odd
 *        polynomial) times 57.29577951308232f in binary32 multiplications, additions and divisions, each rounded
 *        (csrc/terrain.hpp).  +-Inf and denormals are values.
 *      products: a HOST array of n_products (1..7) distinct PCR_HIP_TERRAIN_* ids; dsts, dst_strides: HOST arrays, the band of
 *      each.  src and every dst: `height` rows of `width` floats, strides in floats (any 4-byte alignment; when the rows of all
 *      of them start on 16 bytes the 16-byte accesses are taken).  No dst may overlap src or another dst.  cell sizes and
 *      z_factor finite and not zero.  Argument errors are reported before any HIP call.  Enqueued on s; nothing is allocated
 *      or synchronised. */
enum {
    PCR_HIP_TERRAIN_SLOPE_DEGREES = 0, PCR_HIP_TERRAIN_SLOPE_PERCENT = 1, PCR_HIP_TERRAIN_ASPECT = 2, PCR_HIP_TERRAIN_HILLSHADE = 3,
    PCR_HIP_TERRAIN_TRI = 4, PCR_HIP_TERRAIN_TPI = 5, PCR_HIP_TERRAIN_ROUGHNESS = 6, PCR_HIP_TERRAIN_COUNT = 7
};
int pcr_hip_terrain(const float* src, int width, int height, int64_t src_stride, int n_products, const int* products,
                    float* const* dsts, const int64_t* dst_strides, double cell_size_x, double cell_size_y, double z_factor,
                    int edges, double sin_alt, double ls, double lc, pcr_hip_stream s);

/* ---- individual trees of a canopy band (pcr/core/trees.h: segment_trees; lidR's locate_trees(lmf(ws)) followed by a seeded
 *      descent in the manner of segment_trees(dalponte2016())).  No reference counterpart.  The contract is written once, in
 *      csrc/trees.hpp, which the kernels and the host twin both compile with contraction off; it is comparisons and integer
 *      arithmetic throughout, so they agree bit for bit.
 *        input    one Float32 band H, width x height; a cell that is not finite (NaN, +-Inf) is no data, every other a data
 *                 cell; idx(r, c) = r * width + c; width * height < 2^31
 *        consts   cell = max(|cell_size_x|, |cell_size_y|); k = 0.5 / cell (refused unless finite); M = -1 when
 *                 max_crown_radius is +Inf, else (int64)min(floor((double)max_crown_radius / cell), 2^31 - 1)
 *        order    a beats b when H[a] > H[b], or H[a] == H[b] and idx(a) < idx(b) (binary32 comparisons; -0.0 == +0.0)
 *        window   d = (double)window_base + (double)window_slope * (double)H[c], two rounded operations; rho = d * k;
 *                 R(c) = max_radius_cells if rho >= max_radius_cells, 0 if !(rho >= 1), else (int)rho.  The disc of c: the data
 *                 cells at dr*dr + dc*dc <= R*R inside the image; best(c): its greatest cell, c included
 *        top      a data cell with H[c] >= min_height and best(c) == c; tops are numbered 1..T in increasing idx
 *        crown    set: the tops and every data cell with H[c] >= min_crown_height
 *        parent   of a crown cell: a top is its own; else the greatest of its eight neighbours that are data cells and beat c;
 *                 if there is none, best(c) when that is not c, else c.  root(c): the fixpoint of parent
 *        label    id(root) when root is a top, and c == root or H[c] >= crown_ratio * H[root] (one binary32 multiplication),
 *                 and M < 0 or dr*dr + dc*dc <= M*M in 64-bit integers, (dr, dc) from c to its root; else none
 *        bands    id_dst (float)id, height_dst H[root] bit for bit, both 0x7FC00000 without a label.  Ids above 2^24 are not
 *                 exact in Float32: cells of such trees are 0x7FC00000 in both bands
 *        table    per top in id order: row, col, height = H[top], crown_cells = the cells whose label is the id
 *      Parameter ranges: min_height, min_crown_height finite; window_base, window_slope finite and >= 0; max_radius_cells
 *      1..32; crown_ratio in [0, 1]; max_crown_radius > 0 or +Inf.  Bands: `height` rows of `width` floats, strides in floats,
 *      any 4-byte alignment (rows on 16 bytes take the 16-byte accesses); height_dst may be NULL.  No dst may overlap src, the
 *      other dst or the work area.  d_work: device memory of at least pcr_hip_trees_work_bytes(width, height) bytes (about
 *      12 bytes per cell; answered without a device), the caller's; it carries T, the ids and the crown counts from
 *      pcr_hip_trees to _count and _table.  Argument errors are reported before any HIP call.
 *      pcr_hip_trees: everything is enqueued on s, ceil(log2(width * height)) + 1 pointer-jumping rounds included (a round
 *      returns at once when the one before changed nothing); nothing is allocated or synchronised.
 *      pcr_hip_trees_count: T (and, when asked, how many jumping rounds changed a pointer), after synchronising with s.
 *      pcr_hip_trees_table: rows 0 .. n - 1 of the table into device arrays (any may be NULL), enqueued on s.
 *      pcr_hip_trees_host: the host twin on host arrays, bands and table in one call: *n = T, the first min(T, capacity) rows
 *      are written (n and the arrays may be NULL). */
typedef struct pcr_hip_tree_params {
    float min_height, window_base, window_slope;
    int32_t max_radius_cells;
    float min_crown_height, crown_ratio, max_crown_radius;
    int32_t stop_after;              /* 0: everything.  k = 1..4: pcr_hip_trees enqueues only its first k phases (cells, discs,
                                        numbering, jumping; the labels are the fifth) -- for timing them by difference
                                        (tools/trees_time.py); the bands are then not written */
    double cell_size_x, cell_size_y;
} pcr_hip_tree_params;
int pcr_hip_trees_work_bytes(int width, int height, size_t* bytes);
int pcr_hip_trees(const float* src, int width, int height, int64_t src_stride, const pcr_hip_tree_params* params, float* id_dst,
                  int64_t id_stride, float* height_dst, int64_t height_stride, void* d_work, size_t work_bytes, pcr_hip_stream s);
int pcr_hip_trees_count(const void* d_work, size_t work_bytes, int64_t* n, int* rounds_worked, pcr_hip_stream s);
int pcr_hip_trees_table(const float* src, int width, int height, int64_t src_stride, const void* d_work, size_t work_bytes,
                        int64_t n, int32_t* d_rows, int32_t* d_cols, float* d_heights, int32_t* d_crown_cells, pcr_hip_stream s);
int pcr_hip_trees_host(const float* src, int width, int height, int64_t src_stride, const pcr_hip_tree_params* params,
                       float* id_dst, int64_t id_stride, float* height_dst, int64_t height_stride, int64_t* n, int64_t capacity,
                       int32_t* rows, int32_t* cols, float* heights, int32_t* crown_cells);

/* ---- LAS point records -> the SoA cloud (pcr/io/point_cloud_io.h: LAS input).  No reference counterpart: the reference
 *      declares the format and reads `.las` tiles through laspy in a script.  ASPRS LAS 1.0-1.4, point data record formats
 *      0-10, little-endian, array-of-structures: int32 X, Y, Z, then packed attributes (csrc/las_decode.hpp holds the table).
 *      The raw records cross PCIe (a format-1 record is 28 B, no larger than the cloud it becomes) and are unpacked in HBM.
 *        x = (double)X * scale[0] + offset[0], likewise y: one multiply, one add, each rounded (never an fma)
 *        channels are Float32; z = (float)((double)Z * scale[2] + offset[2]); gps_time = (float)(t - gps_time_origin), the
 *        subtraction in Float64 (Float32 resolves 32 s at 3e8 s); scan_angle in degrees; withheld / overlap 0 or 1
 *      record_length >= the format's minimum (20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67); the excess (extra bytes, and the
 *      wave packets of formats 4, 5, 9, 10) is skipped.
 *      channels: a HOST array of PCR_HIP_LAS_CH_COUNT output pointers, indexed by PCR_HIP_LAS_CH_*; NULL = not wanted (costs
 *      neither the field's extraction nor a store); the array itself may be NULL (x and y alone).
 *      d_records: 16-byte aligned, inside an allocation of at least n * record_length + 16 bytes (the kernel stages a
 *      workgroup's run of records into LDS with aligned 16-byte loads; the last one may reach into the slack, never past it).
 *      A workgroup of 256 lanes owns 256 * PCR_HIP_LAS_RECORDS_PER_LANE consecutive records.  Argument errors (null layout,
 *      format above 10, record_length below the minimum or above 65535, a wanted channel the format lacks, null x / y or
 *      records with n > 0, misaligned records) are reported before any HIP call; n == 0 launches nothing.
 *      _host: the same decoder on host arrays (any alignment, no slack), over `threads` threads (< 1: one). */
typedef struct pcr_hip_las_layout {
    int32_t point_format;
    int32_t record_length;
    double scale[3];
    double offset[3];
    double gps_time_origin;
} pcr_hip_las_layout;
enum {
    PCR_HIP_LAS_CH_Z = 0, PCR_HIP_LAS_CH_INTENSITY = 1, PCR_HIP_LAS_CH_RETURN_NUMBER = 2, PCR_HIP_LAS_CH_NUMBER_OF_RETURNS = 3,
    PCR_HIP_LAS_CH_CLASSIFICATION = 4, PCR_HIP_LAS_CH_WITHHELD = 5, PCR_HIP_LAS_CH_OVERLAP = 6, PCR_HIP_LAS_CH_SCAN_ANGLE = 7,
    PCR_HIP_LAS_CH_USER_DATA = 8, PCR_HIP_LAS_CH_POINT_SOURCE_ID = 9, PCR_HIP_LAS_CH_GPS_TIME = 10, PCR_HIP_LAS_CH_RED = 11,
    PCR_HIP_LAS_CH_GREEN = 12, PCR_HIP_LAS_CH_BLUE = 13, PCR_HIP_LAS_CH_NIR = 14, PCR_HIP_LAS_CH_COUNT = 15
};
#define PCR_HIP_LAS_RECORDS_PER_LANE 4
int pcr_hip_las_decode(const pcr_hip_las_layout* layout, const uint8_t* d_records, uint64_t n, double* d_x, double* d_y,
                       float* const* channels, pcr_hip_stream s);
int pcr_hip_las_decode_host(const pcr_hip_las_layout* layout, const uint8_t* h_records, uint64_t n, double* h_x, double* h_y,
                            float* const* channels, int threads);

/* ---- a band sampled at the points of a cloud: the way back from a raster to the points (pcr/core/sample_grid.h,
 *      PipelineConfig::surface_channels).  No reference counterpart.  The contract is written once, in csrc/sample_grid.hpp,
 *      which the kernel and the host twin both compile with contraction off: they agree bit for bit.
 *        surface   the band's OWN geometry (bounds, signed cell sizes, width, height; tiles and row windows as
 *                  pcr_hip_engine_create wants them, unused here); d_band: height rows of width floats, band_stride floats
 *                  apart.  It need not be the grid the points are rasterised into.
 *        outside   a point outside the inclusive bounds, or with a NaN coordinate, samples NaN; every NaN that leaves is
 *                  0x7FC00000
 *        own cell  (col, row) as the routing answers for that geometry: floor of the true binary64 quotient, then clamp
 *        NEAREST   the own cell's value e
 *        BILINEAR  between cell centres, binary64: qx = (x - min_x) / cell_size_x, tx = (qx - col) - 0.5; tx < 0: neighbour
 *                  column col - 1 with weight wx = -tx, else col + 1 with wx = tx; rows likewise from
 *                  qy = (y - max_y) / cell_size_y.  A neighbour column or row outside the band is replaced by e's own (so
 *                  within half a cell of the border the sample is the 1-D interpolation along the edge); of the cells
 *                  then read (h horizontal, v vertical, d diagonal) a NaN one takes e's value; e NaN: NaN.
 *                  s = ((1-wx)*(1-wy))*e + (wx*(1-wy))*h + ((1-wx)*wy)*v + (wx*wy)*d, added left to right, never an fma
 *        out       d_value == NULL: (float)s (NEAREST: e's bits).  Else (float)((double)value - s), one rounding: the height
 *                  above the surface; a NaN value gives NaN.  +-Inf and denormals are values.
 *      d_out == d_value (in place, z -> height above ground) is allowed; no other overlap of d_out with an input is.  Any
 *      4-byte / 8-byte alignment: when x, y, value and out all start on 16 bytes the 16-byte accesses are taken.  A workgroup
 *      of 256 lanes owns 256 * PCR_HIP_SAMPLE_POINTS_PER_LANE consecutive points.  Argument errors (a grid the engine would
 *      refuse, non-finite geometry, unknown mode, band_stride < width, null band / x / y / out with n > 0, n > 2^40, overlap)
 *      are reported before any HIP call; n == 0 launches nothing.  Enqueued on s; nothing is allocated or synchronised.
 *      _host: the same on host arrays, one thread (callers share the points out: every point is independent). */
#define PCR_HIP_SAMPLE_NEAREST 0
#define PCR_HIP_SAMPLE_BILINEAR 1
#define PCR_HIP_SAMPLE_POINTS_PER_LANE 4
int pcr_hip_sample_grid(const pcr_hip_grid* surface, const float* d_band, int64_t band_stride, const double* d_x,
                        const double* d_y, const float* d_value, uint64_t n, int mode, float* d_out, pcr_hip_stream s);
int pcr_hip_sample_grid_host(const pcr_hip_grid* surface, const float* h_band, int64_t band_stride, const double* h_x,
                             const double* h_y, const float* h_value, uint64_t n, int mode, float* h_out);

/* ---- per-cell histograms: a mergeable piece of state beside the reductions (PipelineConfig::histograms), from which
 *      percentile bands (p95 canopy height, the median) and strata counts come.  No reference counterpart.  The fold is
 *      integer addition: the same bits on both engines and both device paths, for any order, chunking or number of
 *      scatters, with no tolerance anywhere.  The arithmetic is written once, in csrc/histogram.hpp, which the kernels,
 *      the host twin and the host engine compile with contraction off.
 *        accepted   a point is accepted when it is routed to a cell by the rule of the Point glyph (inclusive bounds, the
 *                   floor of the true binary64 quotient, clamp; the owned rows of the engine's grid), is kept by the point
 *                   mask (pcr_hip_engine_set_point_mask), and its value is not NaN.
 *        bin        binary64: the caller computes inv_w = (double)bins / ((double)hi - (double)lo) once;
 *                   t = ((double)v - lo) * inv_w; b = 0 if t < 0, bins - 1 if t >= bins, else (int)t.  Values outside
 *                   [lo, hi) and +-Inf are clamped into the end bins: counted, not dropped.  One subtraction and one
 *                   multiplication: nothing can contract.
 *        state      each accepted point adds 1 to count[b][cell], uint32: a cube of `bins` planes in the state window's
 *                   layout ([bins][state_rows * width]), which the caller zeroes once.  A counter wraps at 2^32: a limit
 *                   that is documented, not checked.
 *        percentile for q, per cell of the owned rows, with N = sum of count[b]: NaN (0x7FC00000) where N == 0 -- the
 *                   touched-tile flags play no part.  Else k = min(max((int64)ceil((double)q * (double)N), 1), N), b the
 *                   smallest bin whose cumulative count C_b >= k, and
 *                   band = (float)(lo + w * ((double)b + ((double)(k - C_{b-1}) - 0.5) / (double)count[b])),
 *                   w = ((double)hi - (double)lo) / bins computed by the caller once, every operation rounded on its own.
 *                   One point in a bin gives the bin's centre; the band is monotone in q.
 *      scatter_histogram honours pcr_hip_engine_set_point_mask and pcr_hip_engine_set_path: 1 direct -- one 32-bit global
 *      atomic add without return per accepted point; 2 binned -- the Point front end on 8-byte records whose value slot
 *      carries the bin, folded in LDS tiles of 128 x h cells x S bin planes, ceil(bins / S) tile launches over records
 *      sorted once; 0 the binned path where it applies, else the direct one.  It sets the touched flags of the tiles its
 *      points are routed to and reports through pcr_hip_engine_stats like pcr_hip_scatter_point.
 *      histogram_percentiles writes n_q bands (own rows x width floats each, d_outs[j] for q[j]; q and d_outs are HOST
 *      arrays) in one launch on s, reading the cube at most twice.  _host: the same lines on host arrays, one thread.
 *      Argument errors -- a null pointer, bins outside 1..256, n_q outside 1..16, q outside [0, 1], non-finite lo, w or
 *      inv_w -- are reported before any HIP call. */
#define PCR_HIP_HISTOGRAM_MAX_BINS 256
#define PCR_HIP_HISTOGRAM_MAX_PERCENTILES 16
int pcr_hip_scatter_histogram(pcr_hip_engine* e, uint32_t* d_counts, int bins, double lo, double inv_w, const double* d_x,
                              const double* d_y, const float* d_value, uint64_t n);
int pcr_hip_histogram_percentiles(const pcr_hip_grid* g, const uint32_t* d_counts, int bins, double lo, double w, int n_q,
                                  const float* q, float* const* d_outs, pcr_hip_stream s);
int pcr_hip_histogram_percentiles_host(const pcr_hip_grid* g, const uint32_t* h_counts, int bins, double lo, double w, int n_q,
                                       const float* q, float* const* h_outs);

/* ---- per-cell extremes: the k lowest (or highest) distinct values of a cell, a mergeable piece of state beside the
 *      reductions (PipelineConfig::extremes), from which an outlier-free Min or Max band comes.  No reference counterpart.
 *      "The k smallest distinct keys" is a set: the same bits on both engines and both device paths, for any order,
 *      chunking or number of scatters, with no tolerance anywhere.  The arithmetic is written once, in csrc/extremes.hpp,
 *      which the kernels, the host twin and the host engine compile with contraction off.
 *        accepted   as for the histograms: a point is accepted when it is routed to a cell by the rule of the Point glyph
 *                   (inclusive bounds, the floor of the true binary64 quotient, clamp; the owned rows of the engine's grid),
 *                   is kept by the point mask (pcr_hip_engine_set_point_mask), and its value is not NaN.  +-Inf are values.
 *        key        the bits of v, -0.0 folded to +0.0 on the bits, then ord(b) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000)
 *                   for LOWEST, ~ord(b) for HIGHEST: the smaller the key the more extreme the value.  Every real value's key
 *                   lies in [0x007FFFFF, 0xFF800000] on either side; EMPTY = 0xFFFFFFFF is above all of them.
 *        state      k planes of uint32 keys in the state window's layout ([k][state_rows * width]), which the caller sets
 *                   to EMPTY once (a byte fill with 0xFF).  After any sequence of scatters plane j of a cell holds the
 *                   (j+1)-th smallest DISTINCT key among the cell's accepted points, or EMPTY.  Distinct values, not
 *                   points: that makes the state a set, hence order-independent; two noise returns at one height count
 *                   as one level.
 *        band       per cell of the owned rows, with n the number of filled slots and v[i] the decoded floats: NaN
 *                   (0x7FC00000) where n == 0 -- the touched-tile flags play no part.  Else start at i = 0 and advance
 *                   while i + 1 < n and d > max_gap, d being ONE binary32 subtraction, v[i+1] - v[i] for LOWEST and
 *                   v[i] - v[i+1] for HIGHEST (distinct keys: never NaN); the band is v[i].  max_gap = +Inf gives the plain
 *                   Min or Max.  A cell whose k kept values are all more than max_gap apart yields the k-th.
 *      scatter_extremes honours pcr_hip_engine_set_point_mask and pcr_hip_engine_set_path: 1 direct -- a displacement
 *      chain of returning 32-bit global atomic minima (at slot j, old = min-exchange of the carried key; stop on a
 *      duplicate; carry the larger of the two on), behind one read of slot k-1 that ends every key that cannot enter;
 *      2 binned -- the Point front end on 8-byte records whose value slot carries the key, the chain on LDS tiles of
 *      128 x h cells x k planes, merged into the state with plain reads and writes where a tile has one owner; 0 the binned
 *      path where it applies, else the direct one.  It sets the touched flags of the tiles its points are routed to and
 *      reports through pcr_hip_engine_stats like pcr_hip_scatter_point.
 *      extremes_band writes the band (own rows x width floats) in one launch on s and, when d_values is not null, the k
 *      decoded planes behind each other ([k][own rows * width] floats, NaN for an empty slot: ascending for LOWEST,
 *      descending for HIGHEST).  _host: the same lines on host arrays, one thread.
 *      Argument errors -- a null pointer, k outside 2..8, an unknown side, a negative or NaN max_gap -- are reported
 *      before any HIP call. */
#define PCR_HIP_EXTREMES_MIN_K 2
#define PCR_HIP_EXTREMES_MAX_K 8
#define PCR_HIP_EXTREMES_LOWEST 0
#define PCR_HIP_EXTREMES_HIGHEST 1
int pcr_hip_scatter_extremes(pcr_hip_engine* e, uint32_t* d_keys, int k, int side, const double* d_x, const double* d_y,
                             const float* d_value, uint64_t n);
int pcr_hip_extremes_band(const pcr_hip_grid* g, const uint32_t* d_keys, int k, int side, float max_gap, float* d_out,
                          float* d_values, pcr_hip_stream s);
int pcr_hip_extremes_band_host(const pcr_hip_grid* g, const uint32_t* h_keys, int k, int side, float max_gap, float* h_out,
                               float* h_values);

/* ---- per-cell stats: the exact mean, variance and standard deviation of a channel per cell, a mergeable piece of state
 *      beside the reductions (PipelineConfig::cell_stats).  No reference counterpart.  The state is three INTEGER planes, so
 *      the fold is integer addition: the same bits on both engines and both device paths, for any order, chunking or number
 *      of scatters, with no tolerance anywhere.  The arithmetic is written once, in csrc/cell_stats.hpp, which the kernels,
 *      the host twin and the host engine compile with contraction off.
 *        accepted   as for the histograms: a point is accepted when it is routed to a cell by the rule of the Point glyph
 *                   (inclusive bounds, the floor of the true binary64 quotient, clamp; the owned rows of the engine's grid),
 *                   is kept by the point mask (pcr_hip_engine_set_point_mask), and its value is not NaN.
 *        step       inv_res = 1.0 / resolution, computed once by the caller.  t = ((double)v - origin) * inv_res, binary64;
 *                   with Q = 2^21: q = -Q if t <= -Q, Q if t >= Q, else (int32)rint(t), ties to even.  Values out of range
 *                   and +-Inf are clamped and COUNTED, like the histogram's end bins.  At a 1 cm step the range is +-20.9 km
 *                   around origin.
 *        state      three planes in the state window's layout ([state_rows * width] each), which the caller zeroes once:
 *                   N (uint32, += 1), S1 (int64, += q), S2 (uint64, += q * q).  S1 cannot wrap while N has not; S2 is exact
 *                   for at least 2^22 accepted points per cell, for 2^32 when |q| <= 2^16; N wraps at 2^32 -- documented,
 *                   not checked, as for the histogram's counters.
 *        bands      per cell of the owned rows, each NaN (0x7FC00000) where N == 0 -- the touched-tile flags play no part:
 *                     MEAN      (float)(origin + resolution * ((double)S1 / (double)N))
 *                     VARIANCE, STDDEV  NaN where N <= ddof; else with D = N * S2 - S1^2, an exact unsigned 128-bit integer
 *                               (hi, lo) (non-negative by Cauchy-Schwarz while nothing has wrapped):
 *                               dd = (double)hi * 0x1p64 + (double)lo;  den = (double)N * (double)(N - ddof);  vq = dd / den;
 *                               VARIANCE = (float)((resolution * resolution) * vq), the product of resolutions computed once;
 *                               STDDEV = (float)(resolution * sqrt(vq)).
 *                   Every operation is rounded on its own; sqrt and / are the correctly rounded binary64 operations.
 *      scatter_cell_stats honours pcr_hip_engine_set_point_mask and pcr_hip_engine_set_path exactly as
 *      pcr_hip_scatter_histogram does: 1 direct -- three no-return global atomic adds per accepted point; 2 binned -- the
 *      Point front end on 8-byte records whose value slot carries the step, two 64-bit LDS atomic adds per record on tiles of
 *      128 x 72 cells, merged into the planes with plain wide reads and writes where a tile has one owner; 0 the binned path
 *      where it applies, else the direct one.  It sets the touched flags of the tiles its points are routed to and reports
 *      through pcr_hip_engine_stats like pcr_hip_scatter_point.
 *      cell_stats_bands writes n_products bands (own rows x width floats each; products[j] names the band d_outs[j] gets) in
 *      one launch on s: one lane per cell reads the three planes coalesced.  _host: the same lines on host arrays, one thread.
 *      Argument errors -- a null pointer, a non-finite origin, a resolution (inv_res) that is not finite and positive, ddof
 *      other than 0 or 1, n_products outside 1..3, an unknown product -- are reported before any HIP call. */
#define PCR_HIP_CELL_STAT_MEAN 0
#define PCR_HIP_CELL_STAT_VARIANCE 1
#define PCR_HIP_CELL_STAT_STDDEV 2
#define PCR_HIP_CELL_STATS_MAX_PRODUCTS 3
#define PCR_HIP_CELL_STATS_Q (1 << 21)
int pcr_hip_scatter_cell_stats(pcr_hip_engine* e, uint32_t* d_n, long long* d_s1, unsigned long long* d_s2, double origin,
                               double inv_res, const double* d_x, const double* d_y, const float* d_value, uint64_t n);
int pcr_hip_cell_stats_bands(const pcr_hip_grid* g, const uint32_t* d_n, const long long* d_s1, const unsigned long long* d_s2,
                             double origin, double resolution, int ddof, int n_products, const int* products, float* const* d_outs,
                             pcr_hip_stream s);
int pcr_hip_cell_stats_bands_host(const pcr_hip_grid* g, const uint32_t* h_n, const long long* h_s1, const unsigned long long* h_s2,
                                  double origin, double resolution, int ddof, int n_products, const int* products,
                                  float* const* h_outs);

/* ---- zonal tables: the per-cell stats planes and histogram cubes above folded by a LABEL BAND into one row per zone
 *      (PipelineConfig::zonal, Pipeline::zonal): per tree with a tree_id band, per plot or stand with a rasterized label grid
 *      -- lidR's crown_metrics and plot_metrics.  No reference counterpart.  The per-cell state is integers, so a zone's state
 *      is the integer sum of its cells': the same bits on both engines for any order or grouping, with no tolerance anywhere.
 *      The arithmetic is written once, in csrc/zonal.hpp, which the kernels, the host twins and the host engine compile with
 *      contraction off.
 *        zone       zone_of(v) = (uint32)v when v is finite, 1 <= v <= 2^24 and v == floorf(v); else 0: no zone (NaN, +-Inf,
 *                   0, -0.0, negatives, 2.5).  Z is the greatest zone of the band (zone_max); a table has rows 0 .. Z - 1, row
 *                   k is zone k + 1; a zone no cell carries has cells = 0.  A zone above the Z passed to a fold is skipped: it is
 *                   never an index.
 *        fold       all counters are 64-bit and wrap modulo 2^64; the caller zeroes the tables.  Per zone:
 *                     cells   uint64, += 1 per cell of the zone
 *                     n, s1, s2   uint64, int64, uint64: += the cell's N (uint32), S1 (int64), S2 (uint64)
 *                     counts[zone][bin]   uint64, += the cell's count[bin][cell] (uint32)
 *        rows, stats   mean, var, std: the per-cell bands' arithmetic ("per-cell stats" above) with a 64-bit n: NaN where
 *                   n == 0, var and std NaN where n <= ddof; D = n * S2 - S1^2 modulo 2^128, one 64 x 64 -> 128 multiply per
 *                   term; dd = (double)hi * 0x1p64 + (double)lo; den = (double)n * (double)(n - ddof); vq = dd / den;
 *                   mean = (float)(origin + resolution * ((double)s1 / (double)n)); var = (float)((resolution * resolution) * vq);
 *                   std = (float)(resolution * sqrt(vq)).
 *        rows, histogram   hist_n = the sum of the zone's bins; per q: NaN where hist_n == 0, else k = min(max((int64)ceil(
 *                   (double)q * (double)hist_n), 1), hist_n), b the smallest bin whose cumulative count C_b >= k, and
 *                   (float)(lo + w * ((double)b + ((double)(k - C_{b-1}) - 0.5) / (double)counts[b])) -- "per-cell histograms"
 *                   above with 64-bit counts (hist_n < 2^63).
 *      Bands and planes are `height` rows of `width` elements, rows `*_stride` ELEMENTS apart (one plane_stride for N, S1 and S2);
 *      the cube's planes are bin_stride elements apart.  Everything is enqueued on s; nothing is allocated.
 *      zone_max: *d_max (one device word, zeroed on s by the call) = Z, or 0 for a band with no zone; a wave reduction, then one
 *      atomic max per wave.  zone_fold_stats: one lane per cell; neighbouring lanes with one zone form a run, a segmented wave
 *      scan sums along it and the run's last lane issues the 64-bit atomic adds (runs go on across a row end of a contiguous
 *      band); a wave with no zone loads nothing further.  d_n, d_s1, d_s2, d_zn, d_zs1, d_zs2 may ALL be null (only cells), or
 *      d_cells may be.  combine = 0 switches the run-combining off -- one set of atomics per cell, for A/B timing and for a test
 *      that both forms give the same bits.  zone_fold_hist: the same lanes, plane after plane; only nonzero counts are added.
 *      zone_rows_stats / zone_rows_percentiles: one lane per zone; a null column is not written; q and d_outs are HOST arrays;
 *      n_q may be 0 (hist_n alone).  _host: the same lines on host arrays, one thread, one add per cell.
 *      Argument errors -- a null pointer, a non-positive size, a stride below the width, bins outside 1..256, Z outside 1..2^24,
 *      more than 2^31 - 1 cells, combine other than 0 or 1, n_q outside 0..16, q outside [0, 1], a table that overlaps an input
 *      or another table -- are reported before any HIP call. */
#define PCR_HIP_ZONE_MAX (1u << 24)
typedef struct pcr_hip_zone_fold_params {
    int32_t combine;                 /* 1: sum along runs of equal zones first; 0: one set of atomics per cell */
    int32_t reserved_;
} pcr_hip_zone_fold_params;
int pcr_hip_zone_max(const float* d_zones, int width, int height, int64_t zone_stride, uint32_t* d_max, pcr_hip_stream s);
int pcr_hip_zone_max_host(const float* h_zones, int width, int height, int64_t zone_stride, uint32_t* max);
int pcr_hip_zone_fold_stats(const float* d_zones, int width, int height, int64_t zone_stride, const uint32_t* d_n, const long long* d_s1,
                            const unsigned long long* d_s2, int64_t plane_stride, uint32_t Z, const pcr_hip_zone_fold_params* params,
                            unsigned long long* d_cells, unsigned long long* d_zn, long long* d_zs1, unsigned long long* d_zs2,
                            pcr_hip_stream s);
int pcr_hip_zone_fold_stats_host(const float* h_zones, int width, int height, int64_t zone_stride, const uint32_t* h_n,
                                 const long long* h_s1, const unsigned long long* h_s2, int64_t plane_stride, uint32_t Z,
                                 const pcr_hip_zone_fold_params* params, unsigned long long* h_cells, unsigned long long* h_zn,
                                 long long* h_zs1, unsigned long long* h_zs2);
int pcr_hip_zone_fold_hist(const float* d_zones, int width, int height, int64_t zone_stride, const uint32_t* d_counts, int bins,
                           int64_t count_stride, int64_t bin_stride, uint32_t Z, const pcr_hip_zone_fold_params* params,
                           unsigned long long* d_zcounts, pcr_hip_stream s);
int pcr_hip_zone_fold_hist_host(const float* h_zones, int width, int height, int64_t zone_stride, const uint32_t* h_counts, int bins,
                                int64_t count_stride, int64_t bin_stride, uint32_t Z, const pcr_hip_zone_fold_params* params,
                                unsigned long long* h_zcounts);
int pcr_hip_zone_rows_stats(const unsigned long long* d_zn, const long long* d_zs1, const unsigned long long* d_zs2, uint32_t Z,
                            double origin, double resolution, int ddof, float* d_mean, float* d_var, float* d_std, pcr_hip_stream s);
int pcr_hip_zone_rows_stats_host(const unsigned long long* h_zn, const long long* h_zs1, const unsigned long long* h_zs2, uint32_t Z,
                                 double origin, double resolution, int ddof, float* h_mean, float* h_var, float* h_std);
int pcr_hip_zone_rows_percentiles(const unsigned long long* d_zcounts, int bins, uint32_t Z, double lo, double w, int n_q, const float* q,
                                  unsigned long long* d_hist_n, float* const* d_outs, pcr_hip_stream s);
int pcr_hip_zone_rows_percentiles_host(const unsigned long long* h_zcounts, int bins, uint32_t Z, double lo, double w, int n_q,
                                       const float* q, unsigned long long* h_hist_n, float* const* h_outs);

/* ---- polygons: a polygon set burnt into a Float32 label band (pcr/core/polygons.h: rasterize_polygons; Pipeline::set_zones
 *      with a PolygonSet) -- gdal_rasterize's cell-centre rule, for the plot and stand maps of the zonal tables above and for
 *      clipping a cloud to an area (the band as a NEAREST surface channel with a filter on it).  No reference counterpart.  The
 *      arithmetic is written once, in csrc/rasterize.hpp, which the kernels and the host twin compile with contraction off: they
 *      agree bit for bit, and both are the per-cell rule below, bit for bit.
 *        input    coords: n_vertices pairs (x, y) of binary64 in the grid's CRS; ring_offsets: n_rings + 1 int64 into the
 *                 vertices; polygon_offsets: n_polygons + 1 int64 into the rings; each starts at 0, does not decrease and ends
 *                 at the count it indexes.  A ring is closed implicitly (a repeated last vertex is a degenerate edge: harmless).
 *                 A polygon is ALL of its rings under the even-odd rule: holes and the parts of a multipolygon are further
 *                 rings, orientation plays no part.  values: n_polygons floats, or NULL for (float)(p + 1).  All HOST arrays.
 *        centre   cx(c) = min_x + (c + 0.5) * cell_size_x, cy(r) = max_y + (r + 0.5) * cell_size_y -- GridConfig::cell_to_world's
 *                 expression: c + 0.5 exact, one rounded product, one rounded sum.  Of the grid only min_x, max_y, the cell
 *                 sizes (either sign), width and height are read.
 *        edge     the endpoints of an edge are ordered so that a.y <= b.y: two polygons that share an edge compute the same bits
 *                 whichever way each walks it.  The edge crosses row r when a.y <= cy(r) < b.y -- half-open: a horizontal edge
 *                 crosses nothing.  Then t = (cy - a.y) / (b.y - a.y) (true division), xc = a.x + t * (b.x - a.x), every
 *                 operation rounded once, never an fma.
 *        inside   cell (r, c) is inside polygon p when the number of p's crossing edges of row r with xc > cx(c) is odd.  So a
 *                 polygon is closed on its low-x and low-y sides and open on the high ones, in world coordinates, and polygons
 *                 that share edges (the same vertex bits) and partition a region label each of its cell centres exactly once.
 *        overlap  the greatest polygon index wins (GDAL's burn order), whatever the order of execution
 *        out      `height` rows of `width` floats, out_stride floats apart: the winning polygon's value, or `background`
 *                 (bit for bit; the project's NaN 0x7FC00000 by default) where no polygon covers the centre
 *      Refused, before any HIP call and with the same message on both paths: a null argument; null or inconsistent offsets; a
 *      ring of fewer than 3 vertices; a coordinate that is not finite or beyond 1e100 in magnitude (so that no intermediate
 *      overflows); more than 2^31 - 2 polygons, or 2^30 edges in one; a grid of more than 2^31 - 1 cells, or whose origin or cell sizes are not finite
 *      or zero; out_stride < width; an output that overlaps an input or the work area; work_bytes below
 *      pcr_hip_rasterize_work_bytes(n_vertices, n_polygons, width, height) (4 bytes per cell + 32 per vertex + 44 per polygon;
 *      answered without a device).  A polygon wholly outside the grid, or of zero area, labels nothing and is no error.
 *      pcr_hip_rasterize_polygons: the host reads every vertex once (the checks, the ordered edges, each polygon's rows and
 *      columns), the tables go to d_work on s and s is waited for ONCE, before the kernels -- the tables leave host memory that
 *      ends with the call.  Then, enqueued on s with nothing allocated: k_poly_fill, one wave per (polygon, row) -- lanes stride
 *      over the polygon's edges, a crossing toggles bit k (the first column the crossing does not count for, found from an
 *      estimate corrected by comparing real cx values) of a per-wave LDS bitmap, PCR_HIP_RASTERIZE_BLOCK_COLS columns of the
 *      polygon's box per pass, then a lane per cell and one global atomic max of p + 1 into a uint32 plane per inside cell;
 *      and k_poly_values, the plane into the band.  params->events: when not NULL, events (pcr_hip_event_create) recorded on s
 *      before k_poly_fill, between the kernels and behind k_poly_values, for timing them (tools/rasterize_time.py).
 *      _host: the same on a host band, one thread, polygons in index order. */
#define PCR_HIP_RASTERIZE_BLOCK_COLS 4096
typedef struct pcr_hip_rasterize_params {
    float background;                /* the bits cells outside every polygon get */
    int32_t reserved_;
    void* events[3];                 /* NULL, or events to record: before k_poly_fill, between the kernels, at the end */
} pcr_hip_rasterize_params;
int pcr_hip_rasterize_work_bytes(int64_t n_vertices, int64_t n_polygons, int width, int height, size_t* bytes);
int pcr_hip_rasterize_polygons(const pcr_hip_grid* grid, const double* h_coords, int64_t n_vertices, const int64_t* h_ring_offsets,
                               int64_t n_rings, const int64_t* h_polygon_offsets, int64_t n_polygons, const float* h_values,
                               const pcr_hip_rasterize_params* params, float* d_out, int64_t out_stride, void* d_work, size_t work_bytes,
                               pcr_hip_stream s);
int pcr_hip_rasterize_polygons_host(const pcr_hip_grid* grid, const double* h_coords, int64_t n_vertices, const int64_t* h_ring_offsets,
                                    int64_t n_rings, const int64_t* h_polygon_offsets, int64_t n_polygons, const float* h_values,
                                    const pcr_hip_rasterize_params* params, float* h_out, int64_t out_stride);

/* ---- polygon index: which polygon holds each POINT of a cloud, exactly (pcr/core/polygons.h: points_in_polygons) -- the clip
 *      and the tagging that the label band above gives only at cell resolution (PDAL filters.crop / filters.overlay).  No
 *      reference counterpart.  The rule is written once, in csrc/point_in_polygon.hpp, on rasterize.hpp's own edge arithmetic,
 *      and compiled by the kernel, the host twin and the index builder with contraction off: they agree bit for bit.
 *        input    the polygon arrays of pcr_hip_rasterize_polygons, with its refusals; a point is (x, y) in binary64 in the
 *                 polygons' CRS
 *        edge     endpoints ordered so that a.y <= b.y; the edge crosses the point's level when a.y <= y < b.y (a horizontal
 *                 edge never does); then xc = a.x + ((y - a.y) / (b.y - a.y)) * (b.x - a.x), every operation rounded once
 *        inside   the point is inside polygon p when the number of p's crossing edges with xc > x is odd, all rings together: a
 *                 polygon is closed on its low-x and low-y sides and open on the high ones, and polygons that share edges (the
 *                 same vertex bits) and partition a region hold every point of it exactly once
 *        overlap  the greatest polygon index wins
 *        out      Float32: values[p] or (float)(p + 1) of the winner; `background` (any bits, kept; default the project's NaN
 *                 0x7FC00000) where no polygon holds the point.  A NaN coordinate is in no polygon; x = -Inf counts every
 *                 crossing, an even number; x = +Inf and y = +-Inf count none.
 *        grid     at a cell centre (cx(c), cy(r)) the answer is the band of pcr_hip_rasterize_polygons on that grid, bit for bit
 *      The index is an accelerator and no part of the contract: a uniform grid of cols x rows cells over the vertices' bounding
 *      box, built on the host (csrc/point_in_polygon_index.hpp, the one builder).  A cell lists, by polygon index descending,
 *      the polygons that hold all of it (no edges) and those with an edge near it (a run of edges to count crossings over); a
 *      walk stops at the first polygon that holds the point.  index_cols / index_rows: 0 automatic (2 * sqrt(vertices) a side,
 *      1 .. 2048), or 1 .. 2048; an automatic side is halved until the tables fit max_index_bytes (0: 256 MiB), an explicit
 *      size that does not fit is refused; either is halved where a cell is narrower than binary64's spacing (info tells).
 *      _create: a host object, no HIP call.  _upload: the tables to d_tables (`bytes` >= _info's bytes) on s, which is waited for
 *      ONCE.  pcr_hip_points_in_polygons: k_points_in_polygons on s, nothing allocated, no host wait: one pass, x and y read and
 *      out stored non-temporally, 16 bytes wide where all three start on 16 bytes; a point whose cell lists more than 16 edges
 *      for a polygon hands that walk to a whole wave through a queue in LDS; events: NULL, or two events (either may be
 *      NULL) recorded before and behind the kernel.  _host: the same walk on host arrays over `threads` threads; every point is
 *      independent, so the bits do not depend on the count.
 *      Refused, before any HIP call and with the same message on both paths: what pcr_hip_rasterize_polygons refuses about the
 *      polygon arrays; a null argument; index_cols or index_rows outside 0 .. 2048; tables over the cap; bytes too small; more
 *      than 2^40 points; an output that overlaps x, y or the tables.  n == 0 is no error.  Polygons with no ring, no area or no
 *      edge hold nothing.  Not done: all_touched, lines and points as geometries, reprojection of the polygons. */
#define PCR_HIP_POLYGON_POINTS_PER_LANE 4
typedef struct pcr_hip_polygon_index pcr_hip_polygon_index;
typedef struct pcr_hip_polygon_index_params {
    float background;                /* the bits points outside every polygon get */
    int32_t index_cols, index_rows;  /* 0: automatic; 1 .. 2048 */
    int32_t reserved_;
    size_t max_index_bytes;          /* 0: 256 MiB */
} pcr_hip_polygon_index_params;
int pcr_hip_polygon_index_create(const double* h_coords, int64_t n_vertices, const int64_t* h_ring_offsets, int64_t n_rings,
                                 const int64_t* h_polygon_offsets, int64_t n_polygons, const float* h_values,
                                 const pcr_hip_polygon_index_params* params, pcr_hip_polygon_index** index);
int pcr_hip_polygon_index_destroy(pcr_hip_polygon_index* index);
int pcr_hip_polygon_index_info(const pcr_hip_polygon_index* index, int* cols, int* rows, int64_t* items, int64_t* listed_edges,
                               size_t* bytes);
int pcr_hip_polygon_index_upload(const pcr_hip_polygon_index* index, void* d_tables, size_t bytes, pcr_hip_stream s);
int pcr_hip_points_in_polygons(const pcr_hip_polygon_index* index, const void* d_tables, const double* d_x, const double* d_y, uint64_t n,
                               float* d_out, pcr_hip_stream s, void* const* events);
int pcr_hip_points_in_polygons_host(const pcr_hip_polygon_index* index, const double* h_x, const double* h_y, uint64_t n, float* h_out,
                                    int threads);

/* ---- point zonal tables: a value channel folded by a per-point LABEL CHANNEL into one row per zone (PipelineConfig::
 *      point_zonal, Pipeline::point_zonal, pcr.point_zonal) -- lidR's plot_metrics and crown_metrics as what they are, a group-by
 *      over POINTS: the zonal tables above give a return the zone of its cell, these give it the zone of its own label (a
 *      polygon channel: exactly the plot that holds it; a Nearest surface channel over a tree_id band; point_source_id: one row
 *      per flight line).  No reference counterpart.  The arithmetic is written once, in csrc/point_zonal.hpp, which the kernels,
 *      the host twins and the host engine compile with contraction off.
 *        zone       of a point: zone_of(label) of the zonal tables above, a whole number in [1, 2^24]; NaN, +-Inf, 0, -0.0,
 *                   negatives and fractions are no zone.  A table has capacity Z: rows 0 .. Z - 1, row k is zone k + 1.  A zone
 *                   above Z is never an index; each point with such a zone that its mask keeps adds 1 to info[1].
 *        accepted   a point whose mask byte is nonzero (or d_mask is NULL), whose zone is in 1..Z and whose value is not NaN
 *                   (cs::kNoStep, hist::kNoBin).  THE GRID PLAYS NO PART: neither x nor y is read, a point outside any grid
 *                   but inside a plot counts.
 *        fold       every counter is 64-bit and wraps modulo 2^64; the caller owns the tables and they ACCUMULATE across calls.
 *                     points[zone]   uint64, += 1 per point with a nonzero mask byte and a zone in 1..Z, whatever its value
 *                     n, s1, s2      per accepted point, q = step_of(v, origin, inv_res) of "per-cell stats": n += 1,
 *                                    s1 += q (int64), s2 += q * q (uint64)
 *                     counts[zone][bin_of(v, lo, inv_w, bins)] += 1 per accepted point ("per-cell histograms")
 *                   Integer addition: any order, chunking, path or engine gives the same bits.
 *        info       two uint64 words the caller owns, accumulated like the tables: info[0] = max(info[0], the greatest zone <= Z
 *                   that a mask-kept point carried), info[1] += the overflow count.  NULL: not kept.
 *        rows       pcr_hip_zone_rows_stats and pcr_hip_zone_rows_percentiles as they are; row k is zone k + 1, up to info[0].
 *      Kernels (csrc/point_zonal.hip), on s, nothing allocated: persistent workgroups of PCR_HIP_POINT_FOLD_BLOCK lanes stride
 *      over tiles of BLOCK * POINTS_PER_LANE points, TILES_IN_FLIGHT tiles loaded before the first is used; label (4 B), mask
 *      (1 B) and value (4 B) are each read once, non-temporally, 16 / 4 / 16 bytes wide per lane where label and value start on
 *      16 bytes and the mask on 4, else element by element.  In a wave neighbouring lanes with one zone (one zone and bin)
 *      form a run; a segmented scan sums along it and its last lane adds the sums to the row:
 *        path 1   with 64-bit global atomic adds, nothing returned -- any Z;
 *        path 2   with LDS atomics into a workgroup-private table (zeroed at the start; a stats row is n << 43 | sum of (q + 2^21),
 *                 S2, and a 32-bit point count -- PCR_HIP_POINT_FOLD_STATS_ROW_BYTES; a histogram row is bins 32-bit counters),
 *                 whose nonzero entries are added to HBM at the end of the workgroup's sweep and after every 2^20 points it has
 *                 read, which bounds the packed and 32-bit fields.  An argument error when Z rows exceed
 *                 PCR_HIP_POINT_FOLD_LDS_BYTES;
 *        path 0   path 2 where it fits, else path 1.
 *      blocks: 0, or the number of workgroups (for timing); never more than there are trips.  info costs one wave reduction and
 *      at most one atomic max and one atomic add per workgroup.  d_value, d_zn, d_zs1 and d_zs2 may ALL be null: `points` only.
 *      pcr_hip_point_fold_plan answers what a call would launch: the path taken, the workgroups, the LDS bytes per workgroup.
 *      _host: one thread, one add per point.  Argument errors -- a null pointer, bins outside 1..256, Z outside 1..2^24, a
 *      non-finite or non-positive constant, a path outside 0..2 or one that does not fit, blocks outside 0..65536, more than 2^40
 *      points, tables that overlap each other or an input -- are reported before any HIP call.  n == 0 changes nothing. */
#define PCR_HIP_POINT_FOLD_BLOCK 256
#define PCR_HIP_POINT_FOLD_POINTS_PER_LANE 4
#define PCR_HIP_POINT_FOLD_TILES_IN_FLIGHT 4
#define PCR_HIP_POINT_FOLD_LDS_BYTES 61440
#define PCR_HIP_POINT_FOLD_STATS_ROW_BYTES 20
#define PCR_HIP_POINT_FOLD_BLOCKS_PER_CU_GLOBAL 8
#define PCR_HIP_POINT_FOLD_BLOCKS_PER_CU_LDS 4
typedef struct pcr_hip_point_fold_params {
    int32_t path;                    /* 0 auto, 1 global atomics, 2 a workgroup-private table in LDS */
    int32_t blocks;                  /* 0: by path and CU count; else the persistent workgroups to launch */
} pcr_hip_point_fold_params;
int pcr_hip_point_fold_plan(uint32_t Z, int bins, uint64_t n, const pcr_hip_point_fold_params* params, int* path, int* blocks,
                            size_t* lds_bytes);
int pcr_hip_point_fold_stats(const float* d_label, const uint8_t* d_mask, const float* d_value, uint64_t n, double origin, double inv_res,
                             uint32_t Z, const pcr_hip_point_fold_params* params, unsigned long long* d_points, unsigned long long* d_zn,
                             long long* d_zs1, unsigned long long* d_zs2, unsigned long long* d_info, pcr_hip_stream s);
int pcr_hip_point_fold_stats_host(const float* h_label, const uint8_t* h_mask, const float* h_value, uint64_t n, double origin,
                                  double inv_res, uint32_t Z, const pcr_hip_point_fold_params* params, unsigned long long* h_points,
                                  unsigned long long* h_zn, long long* h_zs1, unsigned long long* h_zs2, unsigned long long* h_info);
int pcr_hip_point_fold_hist(const float* d_label, const uint8_t* d_mask, const float* d_value, uint64_t n, int bins, double lo, double inv_w,
                            uint32_t Z, const pcr_hip_point_fold_params* params, unsigned long long* d_zcounts, unsigned long long* d_info,
                            pcr_hip_stream s);
int pcr_hip_point_fold_hist_host(const float* h_label, const uint8_t* h_mask, const float* h_value, uint64_t n, int bins, double lo,
                                 double inv_w, uint32_t Z, const pcr_hip_point_fold_params* params, unsigned long long* h_zcounts,
                                 unsigned long long* h_info);

/* ---- polygonize: the zones of a Float32 label band as outlines (pcr/core/polygons.h: polygonize; Pipeline::polygonize) -- the
 *      inverse of "polygons" above, gdal_polygonize's 4-connected rule: crowns from a tree-id band, a zone map as polygons.  No
 *      reference counterpart.  The rule is written once, in csrc/polygonize.hpp, which the kernels and the host twin compile:
 *      they agree bit for bit, and burning the result back with pcr_hip_rasterize_polygons on the same geometry gives the band's
 *      zones cell for cell.
 *        zone     "zonal tables"' rule: the band's value when it is a whole number in [1, 2^24]; NaN of any payload, +-Inf, 0,
 *                 negatives, fractions, values above 2^24 and cells outside the band are no zone
 *        lattice  corner (i, j), i in 0..height, j in 0..width; cell (r, c) has the corners (r, c), (r, c+1), (r+1, c+1), (r+1, c)
 *        edge     side s of a zone cell -- 0 top, 1 right, 2 bottom, 3 left -- is a boundary edge when the cell across it has
 *                 another zone or none.  It is directed with the cell on its right hand in (row-down, column-right) index space:
 *                 top towards +column, right towards +row, bottom towards -column, left towards -row.  Its slot is
 *                 4 * (r * width + c) + s, a uint32.
 *        next     F = the unit step of direction s, O = that of direction (s + 3) % 4, the outward normal; ahead = the zone of
 *                 cell + F, diag = that of cell + F + O.  ahead != z: (r, c, (s + 1) % 4), a right turn, also at a saddle
 *                 (diag == z): regions are 4-connected.  Else diag == z: (cell + F + O, (s + 3) % 4), a left turn.  Else
 *                 (cell + F, s), straight on.  A permutation of each zone's boundary edges whose cycles are the rings: simple
 *                 lattice polygons; rings of one zone may touch at corners and never share an edge.
 *        corner   an edge whose predecessor has another side number.  A ring's vertices are the start corners of its corner
 *                 edges in cycle order, starting at the corner edge of smallest slot, the ring's key: at least 4, no three
 *                 consecutive ones collinear.
 *        table    R rings by ascending key: ring_zone[R] uint32, ring_offset[R + 1] int64 into the V vertices,
 *                 vertex_row[V] and vertex_col[V] int32 lattice corners.  No geometry crosses this interface: the caller groups
 *                 the rings by zone (stable, so a polygon's rings stay in key order; a polygon is all rings of its zone under
 *                 the even-odd rule, holes and parts unmarked) and places corner (i, j) at x = min_x + (double)j * cell_size_x,
 *                 y = max_y + (double)i * cell_size_y, one rounded product and one rounded sum each.
 *      Refused, before any HIP call and with the same message by the host twin: a null argument; a non-positive width or height;
 *      a stride below the width; more than 2^30 - 1 cells (slots fit 32 bits with a sentinel to spare); a work area below its
 *      _work_bytes, or one that overlaps the band or the other; outputs that overlap an input, a work area or each other.  A band
 *      without any zone has E = 0 and is no error: the caller stops there.
 *      Everything is enqueued on s; nothing is allocated; only _count waits.  In order:
 *      pcr_hip_polygonize_edges: d_cells_work, the caller's, of pcr_hip_polygonize_cells_work_bytes(width, height) bytes (2 per
 *      cell; answered without a device): per cell its boundary sides and its edges' place in the compact edge list, which is in
 *      slot order; E.
 *      pcr_hip_polygonize_count: after synchronising with s, E, and once _rings ran R, V and the number of rounds of each
 *      doubling phase that changed something (at most ceil(log2 E) + 1 each).  Any but n_edges may be NULL.
 *      pcr_hip_polygonize_rings: n_edges = E >= 1; d_rings_work of pcr_hip_polygonize_rings_work_bytes(E) bytes (29 per edge).
 *      Per edge its successor and corner flag; the ring keys by minimum-doubling over the cycles (m = min(m, m[j]), j = j[j] from
 *      one buffer into another, ceil(log2 E) + 1 rounds, a round returning at once when the one before lowered no m); the
 *      vertex ranks by a second doubling over the cycles cut at their key edges; R and V by a scan over the key edges.  No
 *      result depends on the order of execution; the only atomic is the relaxed store of 1 into a round's "changed" word.
 *      params: NULL, or events (pcr_hip_event_create) recorded on s behind the edge list, the key rounds, the rank rounds and
 *      the scan (tools/polygonize_time.py).
 *      pcr_hip_polygonize_fetch: n_rings = R and n_vertices = V as _count gave them; the table into the caller's DEVICE arrays.
 *      pcr_hip_polygonize_host: the twin on host arrays, one thread: slots in ascending order, every unvisited corner edge's
 *      cycle walked with the successor rule -- another algorithm than the kernels'.  The counts always; the table when R <=
 *      ring_capacity and V <= vertex_capacity (the arrays may be NULL). */
typedef struct pcr_hip_polygonize_params {
    void* events[4];                 /* NULL, or events to record: behind the edge list, the key rounds, the rank rounds, the scan */
} pcr_hip_polygonize_params;
int pcr_hip_polygonize_cells_work_bytes(int width, int height, size_t* bytes);
int pcr_hip_polygonize_rings_work_bytes(int64_t n_edges, size_t* bytes);
int pcr_hip_polygonize_edges(const float* d_band, int width, int height, int64_t stride, void* d_cells_work, size_t cells_work_bytes,
                             pcr_hip_stream s);
int pcr_hip_polygonize_count(const void* d_cells_work, size_t cells_work_bytes, int64_t* n_edges, int64_t* n_rings, int64_t* n_vertices,
                             int* key_rounds_worked, int* rank_rounds_worked, pcr_hip_stream s);
int pcr_hip_polygonize_rings(const float* d_band, int width, int height, int64_t stride, const void* d_cells_work, size_t cells_work_bytes,
                             int64_t n_edges, void* d_rings_work, size_t rings_work_bytes, const pcr_hip_polygonize_params* params,
                             pcr_hip_stream s);
int pcr_hip_polygonize_fetch(const float* d_band, int width, int height, int64_t stride, const void* d_cells_work, size_t cells_work_bytes,
                             int64_t n_edges, void* d_rings_work, size_t rings_work_bytes, int64_t n_rings, int64_t n_vertices,
                             uint32_t* d_ring_zone, int64_t* d_ring_offset, int32_t* d_vertex_row, int32_t* d_vertex_col,
                             pcr_hip_stream s);
int pcr_hip_polygonize_host(const float* h_band, int width, int height, int64_t stride, int64_t* n_edges, int64_t* n_rings,
                            int64_t* n_vertices, int64_t ring_capacity, int64_t vertex_capacity, uint32_t* h_ring_zone,
                            int64_t* h_ring_offset, int32_t* h_vertex_row, int32_t* h_vertex_col);

#ifdef __cplusplus
}
#endif
#endif
