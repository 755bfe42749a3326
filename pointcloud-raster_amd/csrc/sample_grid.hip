// sample_grid.hip -- pcr_hip_sample_grid / pcr_hip_sample_grid_host (include/pcr_hip.h): one Float32 band sampled at the
// points of a cloud (the contract: sample_grid.hpp), the kernel and its host twin.
//
// One pass over the points; a workgroup of 256 lanes owns kPointsPerBlock = 1024 consecutive points, a lane four of them.
//   1  x, y and the value channel are read once with non-temporal loads, the output is stored non-temporally: neither
//      displaces the band.  VEC (x, y, value and out all start on 16 bytes): a lane owns points 4 t .. 4 t + 3 of the
//      workgroup's run -- two 16-byte loads of x, two of y, one of the value, one 16-byte store; the ragged last quad of the
//      cloud goes point by point.  Otherwise (windows of larger buffers) a lane owns points t, t + 256, t + 512, t + 768 and
//      every access is one element wide.
//   2  the taps of all four points are worked out, then ALL their band loads are issued -- four for Nearest, sixteen for
//      Bilinear -- before the first is used: the gather's latency (an L2 miss into the Infinity Cache for a band beyond an
//      XCD's L2) is paid once per lane, not once per point.  The band is read through ordinary cached loads.  Every tap index
//      is inside the band for every point (sample_grid.hpp: Taps), so the loads need no branch.
//   3  the samples are combined with the contract's lines and leave.
// Nearest is an instantiation of its own (one load per point, no division: the own cell comes from common.hpp's
// world_to_cell); Bilinear takes the two true divisions the contract's fractions need.  No LDS, no atomics, no scratch.
// In place (out == value) is safe: a lane has read the values of its four points before it stores them, and no other lane
// reads them.
#include "common.hpp"
#include "sample_grid.hpp"

#include <cmath>

namespace pcrhip {
namespace {

using namespace sample;

constexpr int kBlock = 256;
constexpr int kPer = PCR_HIP_SAMPLE_POINTS_PER_LANE;
constexpr int kPointsPerBlock = kBlock * kPer;
static_assert(kPer == 4, "the 16-byte accesses of the VEC variant cover four points");

struct SampleArgs {
    GridDev g;                 // the surface's geometry (its reciprocals serve Nearest's routing)
    const float* band;
    int64_t stride;
    const double* x;
    const double* y;
    const float* z;            // null: no value channel
    float* out;
    uint64_t n;
};

template <bool BILINEAR, bool HAS_VALUE, bool VEC>
__global__ __launch_bounds__(kBlock) void k_sample_grid(const SampleArgs a) {
    const uint64_t base = (uint64_t)blockIdx.x * kPointsPerBlock;
    const int tid = threadIdx.x;
    const uint64_t first = VEC ? base + (uint64_t)(kPer * tid) : base + (uint64_t)tid;
    constexpr uint64_t step = VEC ? 1 : kBlock;
    const bool quad = VEC && first + kPer <= a.n;              // this lane's four points in 16-byte accesses

    // 1
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double px[kPer], py[kPer];
    float pz[kPer];
    if (quad) {
        const double2 x0 = stream_load(reinterpret_cast<const double2*>(a.x + first));
        const double2 x1 = stream_load(reinterpret_cast<const double2*>(a.x + first + 2));
        const double2 y0 = stream_load(reinterpret_cast<const double2*>(a.y + first));
        const double2 y1 = stream_load(reinterpret_cast<const double2*>(a.y + first + 2));
        px[0] = x0.x; px[1] = x0.y; px[2] = x1.x; px[3] = x1.y;
        py[0] = y0.x; py[1] = y0.y; py[2] = y1.x; py[3] = y1.y;
        if (HAS_VALUE) {
            const float4 z4 = stream_load(reinterpret_cast<const float4*>(a.z + first));
            pz[0] = z4.x; pz[1] = z4.y; pz[2] = z4.z; pz[3] = z4.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const uint64_t i = first + (uint64_t)k * step;
            const bool live = i < a.n;                         // a slot past the cloud: a NaN coordinate, outside, never stored
            px[k] = live ? __builtin_nontemporal_load(a.x + i) : nan;
            py[k] = live ? __builtin_nontemporal_load(a.y + i) : nan;
            if (HAS_VALUE) pz[k] = live ? __builtin_nontemporal_load(a.z + i) : 0.0f;
        }
    }
    if (!HAS_VALUE) {
#pragma unroll
        for (int k = 0; k < kPer; ++k) pz[k] = 0.0f;
    }

    // 2
    const Geom geom{a.g.min_x, a.g.min_y, a.g.max_x, a.g.max_y, a.g.csx, a.g.csy, a.g.W, a.g.H};
    Taps t[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (BILINEAR) {
            locate<true>(geom, px[k], py[k], t[k]);
        } else {
            int col, row;
            if (world_to_cell(a.g, px[k], py[k], col, row)) taps_nearest(col, row, t[k]);
            else taps_outside(t[k]);
        }
    }
    float e[kPer], h[kPer], v[kPer], d[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const float* own_row = a.band + (int64_t)t[k].row * a.stride;
        e[k] = own_row[t[k].col];
        if (BILINEAR) {
            const float* nb_row = a.band + (int64_t)t[k].nrow * a.stride;
            h[k] = own_row[t[k].ncol];
            v[k] = nb_row[t[k].col];
            d[k] = nb_row[t[k].ncol];
        }
    }

    // 3
    float r[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        if (BILINEAR) r[k] = result<HAS_VALUE>(t[k].inside, bilinear(t[k], e[k], h[k], v[k], d[k]), pz[k]);
        else if (HAS_VALUE) r[k] = result<true>(t[k].inside, (double)e[k], pz[k]);
        else r[k] = result_cell(t[k].inside, e[k]);
    }
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

template <bool BILINEAR, bool HAS_VALUE>
void launch(const SampleArgs& a, bool vec, dim3 grid, hipStream_t st) {
    if (vec) hipLaunchKernelGGL((k_sample_grid<BILINEAR, HAS_VALUE, true>), grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL((k_sample_grid<BILINEAR, HAS_VALUE, false>), grid, dim3(kBlock), 0, st, a);
}

bool disjoint(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 + a_bytes <= b0 || b0 + b_bytes <= a0;
}

// What both entry points check, before any HIP call.  *run: there is something to do.
int check_args(const pcr_hip_grid* surface, const float* band, int64_t stride, const double* x, const double* y,
               const float* z, uint64_t n, int mode, float* out, bool* run) {
    *run = false;
    if (int rc = validate_grid(surface)) return rc;
    PCR_REQUIRE(std::isfinite(surface->min_x) && std::isfinite(surface->min_y) && std::isfinite(surface->max_x) &&
                std::isfinite(surface->max_y) && std::isfinite(surface->cell_size_x) && std::isfinite(surface->cell_size_y),
                "sample_grid: the surface's bounds and cell sizes must be finite");
    PCR_REQUIRE(mode == PCR_HIP_SAMPLE_NEAREST || mode == PCR_HIP_SAMPLE_BILINEAR, "sample_grid: mode must be 0 (nearest) or 1 (bilinear)");
    PCR_REQUIRE(stride >= surface->width, "sample_grid: band_stride is smaller than the surface's width");
    if (n == 0) return PCR_HIP_OK;
    PCR_REQUIRE(band && x && y && out, "sample_grid: null array");
    PCR_REQUIRE(n <= ((uint64_t)1 << 40), "sample_grid: more than 2^40 points in one call");
    const uint64_t band_bytes = ((uint64_t)(surface->height - 1) * (uint64_t)stride + (uint64_t)surface->width) * sizeof(float);
    PCR_REQUIRE(disjoint(out, n * sizeof(float), band, band_bytes) && disjoint(out, n * sizeof(float), x, n * sizeof(double)) &&
                disjoint(out, n * sizeof(float), y, n * sizeof(double)) &&
                (!z || z == out || disjoint(out, n * sizeof(float), z, n * sizeof(float))),
                "sample_grid: out overlaps an input (only out == value, in place, is allowed)");
    *run = true;
    return PCR_HIP_OK;
}

Geom geom_of(const pcr_hip_grid& s) {
    return Geom{s.min_x, s.min_y, s.max_x, s.max_y, s.cell_size_x, s.cell_size_y, s.width, s.height};
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" {

int pcr_hip_sample_grid(const pcr_hip_grid* surface, const float* d_band, int64_t band_stride, const double* d_x,
                        const double* d_y, const float* d_value, uint64_t n, int mode, float* d_out, pcr_hip_stream s) {
    bool run = false;
    if (int rc = check_args(surface, d_band, band_stride, d_x, d_y, d_value, n, mode, d_out, &run)) return rc;
    if (!run) return PCR_HIP_OK;
    SampleArgs a;
    a.g = make_grid_dev(*surface);
    a.band = d_band;
    a.stride = band_stride;
    a.x = d_x;
    a.y = d_y;
    a.z = d_value;
    a.out = d_out;
    a.n = n;
    const bool vec = aligned16(d_x) && aligned16(d_y) && aligned16(d_out) && (!d_value || aligned16(d_value));
    const dim3 grid((unsigned)((n + kPointsPerBlock - 1) / kPointsPerBlock));
    hipStream_t st = static_cast<hipStream_t>(s);
    if (mode == PCR_HIP_SAMPLE_BILINEAR) {
        if (d_value) launch<true, true>(a, vec, grid, st);
        else launch<true, false>(a, vec, grid, st);
    } else {
        if (d_value) launch<false, true>(a, vec, grid, st);
        else launch<false, false>(a, vec, grid, st);
    }
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_sample_grid_host(const pcr_hip_grid* surface, const float* h_band, int64_t band_stride, const double* h_x,
                             const double* h_y, const float* h_value, uint64_t n, int mode, float* h_out) {
    bool run = false;
    if (int rc = check_args(surface, h_band, band_stride, h_x, h_y, h_value, n, mode, h_out, &run)) return rc;
    if (!run) return PCR_HIP_OK;
    const Geom g = geom_of(*surface);
    host_points(g, h_band, band_stride, h_x, h_y, h_value, n, mode, h_out);
    return PCR_HIP_OK;
}

}  // extern "C"
