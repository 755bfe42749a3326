// rasterize.hip -- polygons burnt into a Float32 label band (include/pcr_hip.h "polygons").  The
// arithmetic is csrc/rasterize.hpp, which the host twin at the end of this file compiles too.
//
// The host reads every vertex once: it validates, orders every edge (a.y <= b.y, horizontal ones dropped), and finds each
// polygon's rows and columns in the grid.  A work item is (polygon, row); k_poly_fill gives each a wave.  The wave's lanes stride
// over the polygon's edges; a crossing toggles bit k of a per-wave LDS bitmap of the polygon's columns; then each lane takes a
// cell, inside when the set bits at or below it are odd in number, and inside cells issue one global atomic max of index + 1 into
// a uint32 plane -- the greatest index wins whatever the order.  k_poly_values turns the plane into the band.
#include "band_pass.hpp"
#include "rasterize.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace pcrhip {
namespace {

namespace rs = raster;
using u64 = unsigned long long;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kBlockCols = PCR_HIP_RASTERIZE_BLOCK_COLS;   // columns one pass of the bitmap covers: a word per lane
constexpr int kWords = kBlockCols / 64;
static_assert(kWords == 64, "k_poly_fill zeroes one bitmap word per lane");
constexpr int kInFlight = 4;                               // edge loads a lane issues before it tests the first

struct PolyRec {                     // a polygon with at least one work item
    int64_t edge0;                   // its edges: ey, ex[edge0 .. edge0 + edges)
    int32_t edges;
    int32_t r0;                      // its first row; the rows are item0[m + 1] - item0[m]
    int32_t c0, c1;                  // every k of its crossings lies in [c0, c1]: its cells in [c0, c1)
    uint32_t index;                  // polygon index + 1
    uint32_t pad_;
};
// The edges on the device and in the plan: the y pair, which every lane of every row reads, apart from the x pair, which only a
// crossing reads (interleaved, a row's sweep fetched both: profiles/rasterize.md).
struct EdgeY {
    double ay, by;
};
struct EdgeX {
    double ax, bx;
};
static_assert(sizeof(PolyRec) == 32 && sizeof(EdgeY) == 16 && sizeof(EdgeX) == 16, "work area layout");

// ---- the work area: [plane][edges' y][edges' x][recs][item0][values], each piece on 256 bytes
struct Layout {
    size_t plane, ey, ex, recs, item0, values, total;
};
size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
Layout layout_of(int64_t V, int64_t P, int w, int h) {
    Layout l;
    l.plane = 0;
    l.ey = padded((size_t)w * (size_t)h * 4);
    l.ex = l.ey + padded((size_t)V * sizeof(EdgeY));
    l.recs = l.ex + padded((size_t)V * sizeof(EdgeX));
    l.item0 = l.recs + padded((size_t)P * sizeof(PolyRec));
    l.values = l.item0 + padded(((size_t)P + 1) * 8);
    l.total = l.values + padded((size_t)P * 4) + 256;             // (+ 256: the base is moved up to a multiple of 256)
    return l;
}
char* base_of(void* d_work) { return reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(d_work) + 255) & ~(uintptr_t)255); }

// ---- k_poly_fill
struct FillArgs {
    const EdgeY* ey;
    const EdgeX* ex;
    const PolyRec* recs;
    const int64_t* item0;            // [n_recs + 1]
    int64_t n_recs, items;
    rs::Geom g;
    uint32_t* plane;
};

// The LDS accesses of one wave are in order at the LDS; this keeps the compiler from moving them across the phases of a pass
// (zero, toggle, read), where the lanes that write a word are not the lanes that read it.
__device__ __forceinline__ void wave_lds_phase() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(kBlock) void k_poly_fill(const FillArgs a) {
    __shared__ u64 bitmap[kWaves][kWords];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    u64* bits = bitmap[wave];
    const int64_t step = (int64_t)gridDim.x * kWaves;
    for (int64_t item = (int64_t)blockIdx.x * kWaves + wave; item < a.items; item += step) {
        int64_t lo = 0, hi = a.n_recs - 1;                         // the last polygon with item0 <= item (wave-uniform)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (a.item0[mid] <= item) lo = mid;
            else hi = mid - 1;
        }
        const PolyRec rec = a.recs[lo];
        const int r = rec.r0 + (int)(item - a.item0[lo]);
        const double cyr = rs::cy(a.g, r);
        uint32_t* row = a.plane + (int64_t)r * a.g.w;
        for (int b0 = rec.c0; b0 < rec.c1;) {                      // column blocks of a wide bounding box
            const int n = min(kBlockCols, rec.c1 - b0);
            bits[lane] = 0ull;
            wave_lds_phase();
            for (int e0 = 0; e0 < rec.edges; e0 += 64 * kInFlight) {
                double2 y[kInFlight];                             // the loads of kInFlight steps first, then their tests
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) {
                    const int e = e0 + u * 64 + lane;
                    y[u] = e < rec.edges ? *reinterpret_cast<const double2*>(a.ey + rec.edge0 + e) : make_double2(INFINITY, INFINITY);
                }
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) {
                    if (!(y[u].x <= cyr && cyr < y[u].y)) continue;   // (past the end: +Inf <= cy never holds)
                    const double2 x = *reinterpret_cast<const double2*>(a.ex + rec.edge0 + (e0 + u * 64 + lane));
                    const rs::Edge ed{y[u].x, y[u].y, x.x, x.y};
                    const int k = rs::first_col(a.g, rs::crossing_x(ed, cyr));
                    if (k - b0 < n) {                             // k below the block counts for all of it: bit 0
                        const int kk = k <= b0 ? 0 : k - b0;
                        atomicXor(reinterpret_cast<unsigned*>(bits) + (kk >> 5), 1u << (kk & 31));
                    }
                }
            }
            wave_lds_phase();
            bool carry = false;
            for (int j = 0; j * 64 < n; ++j) {
                const u64 word = bits[j];
                if (word != 0ull || carry) {
                    const int at = j * 64 + lane;
                    if (((rs::inside_of(word, carry) >> lane) & 1ull) && at < n)
                        (void)__hip_atomic_fetch_max(row + ((int64_t)b0 + at), rec.index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                carry ^= (__popcll(word) & 1) != 0;
            }
            wave_lds_phase();
            b0 += n;
        }
    }
}

// ---- k_poly_values
struct ValueArgs {
    const uint32_t* plane;
    const float* values;             // null: (float)(index + 1)
    float* out;
    int64_t stride;
    int w, h;
    uint32_t background;
};
__device__ __forceinline__ float value_of(const ValueArgs& a, uint32_t idx) {
    if (idx == 0u) return __uint_as_float(a.background);
    return a.values ? a.values[idx - 1u] : (float)idx;
}
template <bool VEC>                                               // VEC: width % 4 == 0 and the rows of out start on 16 bytes
__global__ __launch_bounds__(kBlock) void k_poly_values(const ValueArgs a) {
    const int64_t c = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * (VEC ? 4 : 1);
    if (c >= a.w) return;
    for (int r = blockIdx.y; r < a.h; r += gridDim.y) {
        const uint32_t* src = a.plane + (int64_t)r * a.w + c;
        float* dst = a.out + (int64_t)r * a.stride + c;
        if (VEC) {
            const uint4 i = *reinterpret_cast<const uint4*>(src);
            *reinterpret_cast<float4*>(dst) = make_float4(value_of(a, i.x), value_of(a, i.y), value_of(a, i.z), value_of(a, i.w));
        } else {
            *dst = value_of(a, *src);
        }
    }
}

// ---- what both entry points do first: every refusal, then the edges and the work items
struct Plan {
    rs::Geom g;
    std::vector<EdgeY> ey;
    std::vector<EdgeX> ex;
    std::vector<PolyRec> recs;
    std::vector<int64_t> item0;      // [recs + 1]
};

bool offsets_ok(const int64_t* o, int64_t n, int64_t last) {
    if (!o || o[0] != 0 || o[n] != last) return false;
    for (int64_t i = 0; i < n; ++i)
        if (o[i] > o[i + 1]) return false;
    return true;
}

int prepare(const pcr_hip_grid* grid, const double* coords, int64_t V, const int64_t* ring_offsets, int64_t R,
            const int64_t* polygon_offsets, int64_t P, const float* values, const pcr_hip_rasterize_params* params, const float* out,
            int64_t out_stride, const void* work, size_t work_bytes, bool device, Plan* plan) {
    const std::string fn = "rasterize_polygons";
    PCR_REQUIRE(grid && params && out && (coords || V == 0) && (!device || work), fn + ": null argument");
    PCR_REQUIRE(V >= 0 && R >= 0 && P >= 0, fn + ": a negative count");
    PCR_REQUIRE(P <= rs::kMaxPolygons, fn + ": more than 2^31 - 2 polygons");
    PCR_REQUIRE(grid->width > 0 && grid->height > 0, fn + ": width and height must be positive");
    PCR_REQUIRE((int64_t)grid->width * grid->height <= 2147483647LL, fn + ": more than 2^31 - 1 cells");
    PCR_REQUIRE(std::isfinite(grid->min_x) && std::isfinite(grid->max_y) && std::isfinite(grid->cell_size_x) &&
                    std::isfinite(grid->cell_size_y) && grid->cell_size_x != 0.0 && grid->cell_size_y != 0.0,
                fn + ": the grid's origin and cell sizes must be finite, the cell sizes not zero");
    PCR_REQUIRE(out_stride >= grid->width, fn + ": out_stride smaller than width");
    PCR_REQUIRE(offsets_ok(ring_offsets, R, V) && offsets_ok(polygon_offsets, P, R), fn + ": null or inconsistent offsets");
    for (int64_t j = 0; j < R; ++j) PCR_REQUIRE(ring_offsets[j + 1] - ring_offsets[j] >= 3, fn + ": a ring of fewer than 3 vertices");
    for (int64_t i = 0; i < 2 * V; ++i)
        PCR_REQUIRE(std::fabs(coords[i]) <= rs::kMaxCoordinate, fn + ": a coordinate is not finite or beyond 1e100");      // (NaN fails)
    {
        const int w = grid->width, h = grid->height;
        const band::Span ob = band::span_of(out, w, h, out_stride);
        bool clash = band::overlap(ob, band::span_of(ring_offsets, (size_t)(R + 1) * 8)) ||
                     band::overlap(ob, band::span_of(polygon_offsets, (size_t)(P + 1) * 8));
        if (V) clash = clash || band::overlap(ob, band::span_of(coords, (size_t)V * 16));
        if (values && P) clash = clash || band::overlap(ob, band::span_of(values, (size_t)P * 4));
        if (device) clash = clash || band::overlap(ob, band::span_of(work, work_bytes));
        PCR_REQUIRE(!clash, fn + ": the output overlaps an input or the work area");
        if (device) PCR_REQUIRE(work_bytes >= layout_of(V, P, w, h).total, fn + ": work_bytes too small (pcr_hip_rasterize_work_bytes)");
    }

    plan->g = rs::Geom{grid->min_x, grid->max_y, grid->cell_size_x, grid->cell_size_y, grid->width, grid->height};
    plan->item0.assign(1, 0);
    plan->ey.reserve((size_t)V);                                   // (one edge per vertex at most)
    plan->ex.reserve((size_t)V);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t v0 = ring_offsets[polygon_offsets[p]], v1 = ring_offsets[polygon_offsets[p + 1]];
        if (v0 == v1) continue;                                    // no ring
        double xmin = coords[2 * v0], xmax = xmin, ymin = coords[2 * v0 + 1], ymax = ymin;
        for (int64_t v = v0; v < v1; ++v) {
            xmin = std::min(xmin, coords[2 * v]);
            xmax = std::max(xmax, coords[2 * v]);
            ymin = std::min(ymin, coords[2 * v + 1]);
            ymax = std::max(ymax, coords[2 * v + 1]);
        }
        PolyRec rec{};
        int r1;
        rs::rows_between(plan->g, ymin, ymax, rec.r0, r1);
        rs::cols_between(plan->g, xmin, xmax, rec.c0, rec.c1);
        if (r1 <= rec.r0 || rec.c1 <= rec.c0) continue;            // outside the grid, or between two rows or two columns
        rec.edge0 = (int64_t)plan->ey.size();
        for (int64_t j = polygon_offsets[p]; j < polygon_offsets[p + 1]; ++j) {
            const int64_t a0 = ring_offsets[j], n = ring_offsets[j + 1] - a0;
            for (int64_t i = 0; i < n; ++i) {
                const double* a = coords + 2 * (a0 + i);
                const double* b = coords + 2 * (a0 + (i + 1 == n ? 0 : i + 1));          // closed implicitly
                if (a[1] == b[1]) continue;                        // horizontal: crosses no row
                const bool up = a[1] < b[1];
                plan->ey.push_back(up ? EdgeY{a[1], b[1]} : EdgeY{b[1], a[1]});
                plan->ex.push_back(up ? EdgeX{a[0], b[0]} : EdgeX{b[0], a[0]});
            }
        }
        const int64_t ne = (int64_t)plan->ey.size() - rec.edge0;
        if (ne == 0) continue;
        PCR_REQUIRE(ne <= (int64_t)1 << 30, fn + ": a polygon of more than 2^30 edges");
        rec.edges = (int32_t)ne;
        rec.index = (uint32_t)(p + 1);
        plan->recs.push_back(rec);
        plan->item0.push_back(plan->item0.back() + (int64_t)(r1 - rec.r0));
    }
    return PCR_HIP_OK;
}

// ---- the host twin's fill: edge by edge into a bitmap of the polygon's box, then row by row; polygons in index order, a later
// one over an earlier
void fill_host(const Plan& plan, const float* values, float* out, int64_t stride) {
    const rs::Geom& g = plan.g;
    std::vector<uint64_t> bits;
    for (size_t m = 0; m < plan.recs.size(); ++m) {
        const PolyRec& rec = plan.recs[m];
        const int rows = (int)(plan.item0[m + 1] - plan.item0[m]), cols = rec.c1 - rec.c0;
        const size_t words = ((size_t)cols + 63) / 64;
        bits.assign((size_t)rows * words, 0);
        for (int64_t e = rec.edge0; e < rec.edge0 + rec.edges; ++e) {
            const rs::Edge ed{plan.ey[(size_t)e].ay, plan.ey[(size_t)e].by, plan.ex[(size_t)e].ax, plan.ex[(size_t)e].bx};
            int ra, rb;
            rs::rows_between(g, ed.ay, ed.by, ra, rb);
            ra = std::max(ra, rec.r0);
            rb = std::min(rb, rec.r0 + rows);
            for (int r = ra; r < rb; ++r) {
                const int k = rs::first_col(g, rs::crossing_x(ed, rs::cy(g, r)));
                if (k >= rec.c1) continue;
                const int kk = k <= rec.c0 ? 0 : k - rec.c0;
                bits[(size_t)(r - rec.r0) * words + (size_t)(kk >> 6)] ^= (uint64_t)1 << (kk & 63);
            }
        }
        const float v = values ? values[rec.index - 1u] : (float)rec.index;
        for (int r = 0; r < rows; ++r) {
            float* row = out + (int64_t)(rec.r0 + r) * stride + rec.c0;
            bool carry = false;
            for (size_t j = 0; j < words; ++j) {
                const uint64_t word = bits[(size_t)r * words + j];
                uint64_t in = rs::inside_of(word, carry);
                carry ^= (__builtin_popcountll(word) & 1) != 0;
                const int n = std::min(64, cols - (int)(j * 64));
                if (n < 64) in &= ((uint64_t)1 << n) - 1;
                for (; in; in &= in - 1) row[j * 64 + (size_t)__builtin_ctzll(in)] = v;
            }
        }
    }
}

uint32_t bits_of(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" {

int pcr_hip_rasterize_work_bytes(int64_t n_vertices, int64_t n_polygons, int width, int height, size_t* bytes) {
    const std::string fn = "rasterize_work_bytes";
    if (int rc = band::check_extent(fn, bytes != nullptr, width, height)) return rc;
    PCR_REQUIRE(n_vertices >= 0 && n_polygons >= 0, fn + ": a negative count");
    PCR_REQUIRE(n_polygons <= rs::kMaxPolygons, fn + ": more than 2^31 - 2 polygons");
    PCR_REQUIRE((int64_t)width * height <= 2147483647LL, fn + ": more than 2^31 - 1 cells");
    *bytes = layout_of(n_vertices, n_polygons, width, height).total;
    return PCR_HIP_OK;
}

int pcr_hip_rasterize_polygons(const pcr_hip_grid* grid, const double* h_coords, int64_t n_vertices, const int64_t* h_ring_offsets,
                               int64_t n_rings, const int64_t* h_polygon_offsets, int64_t n_polygons, const float* h_values,
                               const pcr_hip_rasterize_params* params, float* d_out, int64_t out_stride, void* d_work, size_t work_bytes,
                               pcr_hip_stream s) {
    Plan plan;
    if (int rc = prepare(grid, h_coords, n_vertices, h_ring_offsets, n_rings, h_polygon_offsets, n_polygons, h_values, params, d_out,
                         out_stride, d_work, work_bytes, true, &plan))
        return rc;
    const int w = grid->width, h = grid->height;
    const Layout l = layout_of(n_vertices, n_polygons, w, h);
    char* base = base_of(d_work);
    hipStream_t st = static_cast<hipStream_t>(s);

    FillArgs f{};
    f.ey = reinterpret_cast<const EdgeY*>(base + l.ey);
    f.ex = reinterpret_cast<const EdgeX*>(base + l.ex);
    f.recs = reinterpret_cast<const PolyRec*>(base + l.recs);
    f.item0 = reinterpret_cast<const int64_t*>(base + l.item0);
    f.n_recs = (int64_t)plan.recs.size();
    f.items = plan.item0.back();
    f.g = plan.g;
    f.plane = reinterpret_cast<uint32_t*>(base + l.plane);
    float* d_values = reinterpret_cast<float*>(base + l.values);

    PCR_HIP_TRY(hipMemsetAsync(f.plane, 0, (size_t)w * (size_t)h * 4, st));
    if (f.items > 0) {
        PCR_HIP_TRY(hipMemcpyAsync(base + l.ey, plan.ey.data(), plan.ey.size() * sizeof(EdgeY), hipMemcpyHostToDevice, st));
        PCR_HIP_TRY(hipMemcpyAsync(base + l.ex, plan.ex.data(), plan.ex.size() * sizeof(EdgeX), hipMemcpyHostToDevice, st));
        PCR_HIP_TRY(hipMemcpyAsync(base + l.recs, plan.recs.data(), plan.recs.size() * sizeof(PolyRec), hipMemcpyHostToDevice, st));
        PCR_HIP_TRY(hipMemcpyAsync(base + l.item0, plan.item0.data(), plan.item0.size() * 8, hipMemcpyHostToDevice, st));
        if (h_values) PCR_HIP_TRY(hipMemcpyAsync(d_values, h_values, (size_t)n_polygons * 4, hipMemcpyHostToDevice, st));
        PCR_HIP_TRY(hipStreamSynchronize(st));                    // the tables above leave host memory that ends with this call
    }
    if (params->events[0]) PCR_HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(params->events[0]), st));
    if (f.items > 0) {
        const unsigned blocks = (unsigned)std::min<int64_t>((f.items + kWaves - 1) / kWaves, (int64_t)1 << 22);
        hipLaunchKernelGGL(k_poly_fill, dim3(blocks), dim3(kBlock), 0, st, f);
    }
    if (params->events[1]) PCR_HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(params->events[1]), st));
    ValueArgs v{f.plane, h_values && f.items > 0 ? d_values : nullptr, d_out, out_stride, w, h, bits_of(params->background)};
    const bool vec = w % 4 == 0 && band::aligned16(d_out, out_stride);
    const int64_t per_block = kBlock * (vec ? 4 : 1);
    const dim3 grid_v((unsigned)(((int64_t)w + per_block - 1) / per_block), (unsigned)std::min(h, 65535));
    if (vec) hipLaunchKernelGGL((k_poly_values<true>), grid_v, dim3(kBlock), 0, st, v);
    else hipLaunchKernelGGL((k_poly_values<false>), grid_v, dim3(kBlock), 0, st, v);
    if (params->events[2]) PCR_HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(params->events[2]), st));
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_rasterize_polygons_host(const pcr_hip_grid* grid, const double* h_coords, int64_t n_vertices, const int64_t* h_ring_offsets,
                                    int64_t n_rings, const int64_t* h_polygon_offsets, int64_t n_polygons, const float* h_values,
                                    const pcr_hip_rasterize_params* params, float* h_out, int64_t out_stride) {
    Plan plan;
    if (int rc = prepare(grid, h_coords, n_vertices, h_ring_offsets, n_rings, h_polygon_offsets, n_polygons, h_values, params, h_out,
                         out_stride, nullptr, 0, false, &plan))
        return rc;
    for (int r = 0; r < grid->height; ++r) std::fill_n(h_out + (int64_t)r * out_stride, grid->width, params->background);
    fill_host(plan, h_values, h_out, out_stride);
    return PCR_HIP_OK;
}

}  // extern "C"
