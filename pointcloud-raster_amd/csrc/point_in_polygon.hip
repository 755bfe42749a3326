// point_in_polygon.hip -- pcr_hip_polygon_index_* and pcr_hip_points_in_polygons (include/pcr_hip.h "polygon index", DESIGN.md
// section 26): which polygon holds each point of a cloud, exactly.  The rule and the walk are csrc/point_in_polygon.hpp; the
// index is built on the host by csrc/point_in_polygon_index.hpp, the one builder, which also holds the host twin's loop.
//
// k_points_in_polygons: one pass over the points; a workgroup of 256 lanes owns 1024 consecutive points, a lane four of them.
//   1  x and y are read once with non-temporal loads and the output is stored non-temporally, so the stream does not displace
//      the tables.  VEC (x, y and out all start on 16 bytes): a lane owns points 4 t .. 4 t + 3 -- two 16-byte loads of x, two of
//      y, one 16-byte store; the ragged last quad goes point by point.  Otherwise a lane owns points t, t + 256, t + 512, t + 768
//      and every access is one element wide.
//   2  the cells of all four points are found with bin(), then the eight cell_start loads and then the four first items are issued
//      before any is used: the common lane -- one flagged item, no edges -- pays the tables' latency once, not four times.
//   3  a point walks its cell's items (polygon index descending) and stops at the first polygon that holds it.  For a mixed item
//      of at most kInline edges the lane loops over the item's edges: kInFlight y pairs are loaded before the first test, the x
//      pair only on a crossing.  Every loop bound is a table count.  The tables go through ordinary cached loads.
//   4  a point that meets a LONGER list stops there and is put on a queue in LDS (one LDS atomic; kQueue entries: the point, where
//      its walk stands), and behind a barrier the workgroup's waves take the queued points one each: the wave walks on from that
//      item with its 64 lanes striding over the item's edges, the parity XORed across the lanes with a ballot.  One lane no longer
//      walks hundreds of edges while 63 wait for it (profiles/points_in_polygons.md has the kernel without the queue).  A point
//      that finds the queue full walks its list itself, as in 3: the answer is the same either way, the rule's.
//   5  the answers of the queued points come back through LDS and everything is stored.  7.2 KB of LDS, no scratch.
#include "common.hpp"
#include "point_in_polygon_index.hpp"

#include <cmath>

struct pcr_hip_polygon_index {
    pcrhip::pip::Index ix;
};

namespace pcrhip {
namespace {

namespace rs = raster;

constexpr int kBlock = 256;
constexpr int kPer = PCR_HIP_POLYGON_POINTS_PER_LANE;
constexpr int kPointsPerBlock = kBlock * kPer;
constexpr int kInFlight = 4;                                   // edge loads a lane issues before it tests the first
constexpr int kInline = 16;                                    // a list of at most this many edges is walked by the point's own lane
constexpr int kQueue = 256;                                    // longer lists of a workgroup's points wait here for a whole wave
static_assert(kPer == 4, "the 16-byte accesses of the VEC variant cover four points");

struct PipArgs {
    pip::View v;
    const double* x;
    const double* y;
    float* out;
    uint64_t n;
};

// The parity of the crossings to the right of (x, y) among the `count` edges from `start`: pip::odd_crossings with the loads of
// kInFlight edges issued together.
__device__ __forceinline__ bool odd_crossings_dev(const pip::View& v, uint32_t start, uint32_t count, double x, double y) {
    bool odd = false;
    const pip::EdgeY* ey = v.ey + start;
    const pip::EdgeX* ex = v.ex + start;
    for (uint32_t e0 = 0; e0 < count; e0 += kInFlight) {
        double2 yy[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u)
            yy[u] = e0 + u < count ? *reinterpret_cast<const double2*>(ey + e0 + u) : make_double2(INFINITY, INFINITY);
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            if (!(yy[u].x <= y && y < yy[u].y)) continue;       // (past the end: y < +Inf and +Inf <= y never both hold)
            const double2 xx = *reinterpret_cast<const double2*>(ex + e0 + u);
            const rs::Edge ed{yy[u].x, yy[u].y, xx.x, xx.y};
            if (rs::crossing_x(ed, y) > x) odd = !odd;
        }
    }
    return odd;
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_points_in_polygons(const PipArgs a) {
    __shared__ double q_x[kQueue], q_y[kQueue];
    __shared__ uint32_t q_it[kQueue], q_end[kQueue], q_won[kQueue];
    __shared__ uint32_t q_count;
    const uint64_t base = (uint64_t)blockIdx.x * kPointsPerBlock;
    const int tid = threadIdx.x;
    if (tid == 0) q_count = 0u;
    __syncthreads();
    const uint64_t first = VEC ? base + (uint64_t)(kPer * tid) : base + (uint64_t)tid;
    constexpr uint64_t step = VEC ? 1 : kBlock;
    const bool quad = VEC && first + kPer <= a.n;

    // 1
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double px[kPer], py[kPer];
    if (quad) {
        const double2 x0 = stream_load(reinterpret_cast<const double2*>(a.x + first));
        const double2 x1 = stream_load(reinterpret_cast<const double2*>(a.x + first + 2));
        const double2 y0 = stream_load(reinterpret_cast<const double2*>(a.y + first));
        const double2 y1 = stream_load(reinterpret_cast<const double2*>(a.y + first + 2));
        px[0] = x0.x; px[1] = x0.y; px[2] = x1.x; px[3] = x1.y;
        py[0] = y0.x; py[1] = y0.y; py[2] = y1.x; py[3] = y1.y;
    } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint64_t i = first + (uint64_t)k * step;
            const bool live = i < a.n;                         // a slot past the cloud: NaN, in no polygon, never stored
            px[k] = live ? __builtin_nontemporal_load(a.x + i) : nan;
            py[k] = live ? __builtin_nontemporal_load(a.y + i) : nan;
        }
    }

    // 2
    uint32_t it0[kPer], it1[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int64_t cell = (int64_t)pip::bj(a.v.b, py[k]) * a.v.b.gx + pip::bi(a.v.b, px[k]);
        it0[k] = a.v.cell_start[cell];
        it1[k] = a.v.cell_start[cell + 1];
    }
    uint4 head[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (px[k] != px[k] || py[k] != py[k]) it1[k] = it0[k];   // NaN: no walk
        head[k] = it0[k] < it1[k] ? *reinterpret_cast<const uint4*>(a.v.items + it0[k]) : make_uint4(0u, 0u, 0u, 0u);
    }

    // 3
    uint32_t won[kPer];
    int queued[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        won[k] = 0u;
        queued[k] = -1;
        uint4 item = head[k];
        for (uint32_t it = it0[k]; it < it1[k];) {
            if (item.z == pip::kInside) {
                won[k] = item.x;
                break;
            }
            if (item.z > (uint32_t)kInline) {                      // a long list: to the queue, unless it is full
                const uint32_t slot = atomicAdd(&q_count, 1u);
                if (slot < (uint32_t)kQueue) {
                    q_x[slot] = px[k];
                    q_y[slot] = py[k];
                    q_it[slot] = it;
                    q_end[slot] = it1[k];
                    queued[k] = (int)slot;
                    break;
                }
            }
            if (odd_crossings_dev(a.v, item.y, item.z, px[k], py[k])) {
                won[k] = item.x;
                break;
            }
            if (++it < it1[k]) item = *reinterpret_cast<const uint4*>(a.v.items + it);
        }
    }

    // 4
    __syncthreads();
    const uint32_t in_queue = min(q_count, (uint32_t)kQueue);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (uint32_t q = (uint32_t)wave; q < in_queue; q += kBlock / 64) {
        const double x = q_x[q], y = q_y[q];
        const uint32_t end = __builtin_amdgcn_readfirstlane(q_end[q]);
        uint32_t holder = 0u;
        for (uint32_t it = __builtin_amdgcn_readfirstlane(q_it[q]); it < end; ++it) {
            const uint4 item = *reinterpret_cast<const uint4*>(a.v.items + it);
            const uint32_t count = __builtin_amdgcn_readfirstlane(item.z), start = __builtin_amdgcn_readfirstlane(item.y);
            if (count == pip::kInside) {
                holder = item.x;
                break;
            }
            bool odd = false;
            for (uint32_t e = (uint32_t)lane; e < count; e += 64u) {
                const double2 yy = *reinterpret_cast<const double2*>(a.v.ey + start + e);
                if (!(yy.x <= y && y < yy.y)) continue;
                const double2 xx = *reinterpret_cast<const double2*>(a.v.ex + start + e);
                const rs::Edge ed{yy.x, yy.y, xx.x, xx.y};
                if (rs::crossing_x(ed, y) > x) odd = !odd;
            }
            if (__popcll(__ballot(odd)) & 1) {                     // (XOR over the lanes: the order plays no part)
                holder = item.x;
                break;
            }
        }
        if (lane == 0) q_won[q] = holder;
    }
    __syncthreads();

    // 5
    float r[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) r[k] = pip::value_of(a.v.values, a.v.background, queued[k] >= 0 ? q_won[queued[k]] : won[k]);
    if (quad) {
        __builtin_nontemporal_store(pcr_f4v{r[0], r[1], r[2], r[3]}, reinterpret_cast<pcr_f4v*>(a.out + first));
    } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint64_t i = first + (uint64_t)k * step;
            if (i < a.n) __builtin_nontemporal_store(r[k], a.out + i);
        }
    }
}

bool disjoint(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 + a_bytes <= b0 || b0 + b_bytes <= a0;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
char* base_of(void* d) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(d) + 255) & ~(uintptr_t)255); }

// What both point calls check, before any HIP call.  *run: there is something to do.
int check_points(const pcr_hip_polygon_index* index, const void* tables, bool device, const double* x, const double* y, uint64_t n,
                 const float* out, bool* run) {
    const std::string fn = "points_in_polygons";
    *run = false;
    PCR_REQUIRE(index && (!device || tables), fn + ": null argument");
    if (n == 0) return PCR_HIP_OK;
    PCR_REQUIRE(x && y && out, fn + ": null argument");
    PCR_REQUIRE(n <= ((uint64_t)1 << 40), fn + ": more than 2^40 points in one call");
    bool ok = disjoint(out, n * 4, x, n * 8) && disjoint(out, n * 4, y, n * 8);
    if (device) ok = ok && disjoint(out, n * 4, tables, pip::layout_of(index->ix).total);
    PCR_REQUIRE(ok, fn + ": the output overlaps x, y or the tables");
    *run = true;
    return PCR_HIP_OK;
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" {

int pcr_hip_polygon_index_create(const double* h_coords, int64_t n_vertices, const int64_t* h_ring_offsets, int64_t n_rings,
                                 const int64_t* h_polygon_offsets, int64_t n_polygons, const float* h_values,
                                 const pcr_hip_polygon_index_params* params, pcr_hip_polygon_index** index) {
    const std::string fn = "polygon_index";
    PCR_REQUIRE(params && index, fn + ": null argument");
    pip::BuildParams bp;
    std::memcpy(&bp.background, &params->background, 4);
    bp.cols = params->index_cols;
    bp.rows = params->index_rows;
    bp.max_bytes = params->max_index_bytes;
    pcr_hip_polygon_index* made = new pcr_hip_polygon_index();
    std::string err;
    if (!pip::build_index(h_coords, n_vertices, h_ring_offsets, n_rings, h_polygon_offsets, n_polygons, h_values, bp, &made->ix, &err)) {
        delete made;
        return fail(PCR_HIP_INVALID_ARGUMENT, fn + ": " + err);
    }
    *index = made;
    return PCR_HIP_OK;
}

int pcr_hip_polygon_index_destroy(pcr_hip_polygon_index* index) {
    delete index;
    return PCR_HIP_OK;
}

int pcr_hip_polygon_index_info(const pcr_hip_polygon_index* index, int* cols, int* rows, int64_t* items, int64_t* listed_edges,
                               size_t* bytes) {
    PCR_REQUIRE(index, "polygon_index_info: null argument");
    if (cols) *cols = index->ix.b.gx;
    if (rows) *rows = index->ix.b.gy;
    if (items) *items = (int64_t)index->ix.items.size();
    if (listed_edges) *listed_edges = (int64_t)index->ix.ey.size();
    if (bytes) *bytes = pip::layout_of(index->ix).total;
    return PCR_HIP_OK;
}

int pcr_hip_polygon_index_upload(const pcr_hip_polygon_index* index, void* d_tables, size_t bytes, pcr_hip_stream s) {
    const std::string fn = "polygon_index_upload";
    PCR_REQUIRE(index && d_tables, fn + ": null argument");
    const pip::Index& ix = index->ix;
    const pip::Layout l = pip::layout_of(ix);
    PCR_REQUIRE(bytes >= l.total, fn + ": bytes too small (pcr_hip_polygon_index_info)");
    char* base = base_of(d_tables);
    hipStream_t st = static_cast<hipStream_t>(s);
    PCR_HIP_TRY(hipMemcpyAsync(base + l.cell_start, ix.cell_start.data(), ix.cell_start.size() * 4, hipMemcpyHostToDevice, st));
    if (!ix.items.empty())
        PCR_HIP_TRY(hipMemcpyAsync(base + l.items, ix.items.data(), ix.items.size() * sizeof(pip::Item), hipMemcpyHostToDevice, st));
    if (!ix.ey.empty()) {
        PCR_HIP_TRY(hipMemcpyAsync(base + l.ey, ix.ey.data(), ix.ey.size() * sizeof(pip::EdgeY), hipMemcpyHostToDevice, st));
        PCR_HIP_TRY(hipMemcpyAsync(base + l.ex, ix.ex.data(), ix.ex.size() * sizeof(pip::EdgeX), hipMemcpyHostToDevice, st));
    }
    if (ix.has_values && !ix.values.empty())
        PCR_HIP_TRY(hipMemcpyAsync(base + l.values, ix.values.data(), ix.values.size() * 4, hipMemcpyHostToDevice, st));
    PCR_HIP_TRY(hipStreamSynchronize(st));                         // the copies read pageable host memory: done when this returns
    return PCR_HIP_OK;
}

int pcr_hip_points_in_polygons(const pcr_hip_polygon_index* index, const void* d_tables, const double* d_x, const double* d_y, uint64_t n,
                               float* d_out, pcr_hip_stream s, void* const* events) {
    bool run = false;
    if (int rc = check_points(index, d_tables, true, d_x, d_y, n, d_out, &run)) return rc;
    hipStream_t st = static_cast<hipStream_t>(s);
    if (events && events[0]) PCR_HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(events[0]), st));
    if (run) {
        const pip::Index& ix = index->ix;
        const pip::Layout l = pip::layout_of(ix);
        const char* base = base_of(const_cast<void*>(d_tables));
        PipArgs a;
        a.v.b = ix.b;
        a.v.cell_start = reinterpret_cast<const uint32_t*>(base + l.cell_start);
        a.v.items = reinterpret_cast<const pip::Item*>(base + l.items);
        a.v.ey = reinterpret_cast<const pip::EdgeY*>(base + l.ey);
        a.v.ex = reinterpret_cast<const pip::EdgeX*>(base + l.ex);
        a.v.values = ix.has_values ? reinterpret_cast<const float*>(base + l.values) : nullptr;
        a.v.background = ix.background;
        a.x = d_x;
        a.y = d_y;
        a.out = d_out;
        a.n = n;
        const dim3 grid((unsigned)((n + kPointsPerBlock - 1) / kPointsPerBlock));
        if (aligned16(d_x) && aligned16(d_y) && aligned16(d_out)) hipLaunchKernelGGL((k_points_in_polygons<true>), grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((k_points_in_polygons<false>), grid, dim3(kBlock), 0, st, a);
    }
    if (events && events[1]) PCR_HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(events[1]), st));
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_points_in_polygons_host(const pcr_hip_polygon_index* index, const double* h_x, const double* h_y, uint64_t n, float* h_out,
                                    int threads) {
    bool run = false;
    if (int rc = check_points(index, nullptr, false, h_x, h_y, n, h_out, &run)) return rc;
    if (run) pip::points_host(index->ix, h_x, h_y, n, h_out, threads);
    return PCR_HIP_OK;
}

}  // extern "C"
