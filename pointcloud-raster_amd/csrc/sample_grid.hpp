// sample_grid.hpp -- the per-point arithmetic of sampling one Float32 band at the points of a cloud (pcr_hip_sample_grid,
// pcr::sample_grid, PipelineConfig::surface_channels), for the device (csrc/sample_grid.hip) and the host loop
// (pcr_hip_sample_grid_host): both compile these lines, with contraction off, so a channel gathered in HBM and one gathered by
// the host loop agree bit for bit.
//
// The surface.  One Float32 band of W x H cells, rows `stride` floats apart, with a geometry of its own: min_x, min_y, max_x,
// max_y, signed cell_size_x, signed cell_size_y, origin (min_x, max_y).  It need not be the grid the points are rasterised
// into.  NaN is "no data"; every NaN that leaves these functions is 0x7FC00000.
// Outside.  A point (x, y) with !(min_x <= x <= max_x && min_y <= y <= max_y) -- outside the inclusive bounds, or a NaN
//   coordinate -- samples NaN.
// Own cell.  qx = (x - min_x) / cell_size_x, qy = (y - max_y) / cell_size_y, TRUE binary64 divisions;
//   col = clamp((int)floor(qx), 0, W - 1), row = clamp((int)floor(qy), 0, H - 1): what world_to_cell (csrc/common.hpp,
//   GridConfig::world_to_cell) answers for this geometry, so a point sampled from the grid it was rasterised into reads the
//   cell it contributed to.  e = band[row][col].
// Nearest.   the sample is e.
// Bilinear.  interpolation between cell CENTRES, binary64:
//   tx = (qx - col) - 0.5;  tx < 0: the neighbour column is col - 1 and wx = -tx, else col + 1 and wx = tx
//   ty = (qy - row) - 0.5;  ty < 0: the neighbour row    is row - 1 and wy = -ty, else row + 1 and wy = ty
//   a neighbour column or row outside the band is MISSING and is replaced by e's own (ncol = col, nrow = row); then
//   h = band[row][ncol], v = band[nrow][col], d = band[nrow][ncol], and one of them that is NaN is missing too and takes e's
//   value (the terrain bands' compute_edges rule).  So an outside h or v IS e; the diagonal of a missing row is h, of a
//   missing column v, of both e: within half a cell of the border the sample is the 1-D interpolation along the edge, and
//   in a corner it is e.  e NaN: the sample is NaN
//   s = ((1-wx)*(1-wy))*e + (wx*(1-wy))*h + ((1-wx)*wy)*v + (wx*wy)*d, every product and sum rounded, added left to right,
//   never an fma
// Output, Float32, one rounding:
//   without a value channel   (float)s; Nearest: e's bits, a NaN made canonical
//   with a value channel z    (float)((double)z - s), s = (double)e for Nearest; a NaN z gives NaN
// +-Inf and denormals are ordinary values; a NaN they lead to (0 * Inf, Inf - Inf) is 0x7FC00000 like every other.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCR_SAMPLE_HD __host__ __device__ __forceinline__
#else
#define PCR_SAMPLE_HD inline
#endif

namespace pcrhip {
namespace sample {

// mode ids: PCR_HIP_SAMPLE_* of include/pcr_hip.h, pcr::SampleMode
enum : int { kNearest = 0, kBilinear = 1 };

struct Geom {
    double min_x, min_y, max_x, max_y;
    double csx, csy;
    int W, H;
};

// What one point reads of the band.  The indices are inside the band for EVERY point, so that the loads need no branch: a
// point outside reads cell (0, 0) and drops it (inside == false), a neighbour column or row outside the band is the own one.
struct Taps {
    int col, row;          // own cell
    int ncol, nrow;        // neighbour column and row; the own ones where the band ends
    bool inside;           // the point is inside the bounds
    double wx, wy;         // Bilinear: the neighbours' weights
};

PCR_SAMPLE_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

PCR_SAMPLE_HD bool in_bounds(const Geom& g, double x, double y) {
    return x >= g.min_x && x <= g.max_x && y >= g.min_y && y <= g.max_y;      // false for a NaN coordinate
}

PCR_SAMPLE_HD int clamp_cell(double fl, int n) {
    // (fl is the floor of a finite quotient of a point inside the bounds; the comparison is done before the conversion so
    // that a huge quotient of a degenerate geometry cannot overflow the int)
    return fl < 0.0 ? 0 : fl > (double)(n - 1) ? n - 1 : (int)fl;
}

// A point that is inside the bounds, its own cell known (col, row as above): the Nearest taps.
PCR_SAMPLE_HD void taps_nearest(int col, int row, Taps& t) {
    t.col = t.ncol = col;
    t.row = t.nrow = row;
    t.inside = true;
    t.wx = t.wy = 0.0;
}
PCR_SAMPLE_HD void taps_outside(Taps& t) {
    t.col = t.ncol = t.row = t.nrow = 0;
    t.inside = false;
    t.wx = t.wy = 0.0;
}

// One axis of Bilinear: own index, neighbour index (the own one where the band ends), the neighbour's weight.
PCR_SAMPLE_HD void axis(double q, int n, int& own, int& nb, double& w) {
    own = clamp_cell(__builtin_floor(q), n);
    const double t = (q - (double)own) - 0.5;
    const int want = t < 0.0 ? own - 1 : own + 1;
    w = t < 0.0 ? -t : t;
    nb = want >= 0 && want < n ? want : own;
}

// The taps of any point, from true divisions (the host loop in both modes; the kernel for Bilinear, which needs the
// fractions -- its Nearest instantiation takes the own cell from common.hpp's world_to_cell, which answers the same).
template <bool BILINEAR>
PCR_SAMPLE_HD void locate(const Geom& g, double x, double y, Taps& t) {
    if (!in_bounds(g, x, y)) { taps_outside(t); return; }
    const double qx = (x - g.min_x) / g.csx, qy = (y - g.max_y) / g.csy;
    if (!BILINEAR) {
        taps_nearest(clamp_cell(__builtin_floor(qx), g.W), clamp_cell(__builtin_floor(qy), g.H), t);
        return;
    }
    t.inside = true;
    axis(qx, g.W, t.col, t.ncol, t.wx);
    axis(qy, g.H, t.row, t.nrow, t.wy);
}

// The sample of the four cells read at the taps, as binary64; NaN (any NaN: result() makes it canonical) when e is.
PCR_SAMPLE_HD double bilinear(const Taps& t, float e, float h, float v, float d) {
    if (!(h == h)) h = e;
    if (!(v == v)) v = e;
    if (!(d == d)) d = e;
    const double ux = 1.0 - t.wx, uy = 1.0 - t.wy;
    double s = (ux * uy) * (double)e;
    s = s + (t.wx * uy) * (double)h;
    s = s + (ux * t.wy) * (double)v;
    s = s + (t.wx * t.wy) * (double)d;
    return s;
}

// The channel value of a point: `s` its sample (ignored when !inside), z its value when HAS_VALUE.
template <bool HAS_VALUE>
PCR_SAMPLE_HD float result(bool inside, double s, float z) {
    if (!inside) return nodata();
    const float r = HAS_VALUE ? (float)((double)z - s) : (float)s;
    return r == r ? r : nodata();
}
// Nearest without a value channel: the cell's bits (no conversion: a denormal stays what it is in any denormal mode).
PCR_SAMPLE_HD float result_cell(bool inside, float e) { return inside && e == e ? e : nodata(); }

// ---- the host loop (pcr_hip_sample_grid_host, and any program that compiles this header alone) ------------------------------
template <bool BILINEAR, bool HAS_VALUE>
inline void host_loop(const Geom& g, const float* band, int64_t stride, const double* x, const double* y, const float* z, uint64_t n,
               float* out) {
    for (uint64_t i = 0; i < n; ++i) {
        Taps t;
        locate<BILINEAR>(g, x[i], y[i], t);
        const float* own_row = band + (int64_t)t.row * stride;
        const float e = own_row[t.col];
        const float zi = HAS_VALUE ? z[i] : 0.0f;              // (read before out[i] is stored: out may be z)
        float r;
        if (BILINEAR) {
            const float* nb_row = band + (int64_t)t.nrow * stride;
            r = result<HAS_VALUE>(t.inside, bilinear(t, e, own_row[t.ncol], nb_row[t.col], nb_row[t.ncol]), zi);
        } else if (HAS_VALUE) {
            r = result<true>(t.inside, (double)e, zi);
        } else {
            r = result_cell(t.inside, e);
        }
        out[i] = r;
    }
}

// n points of checked arguments (include/pcr_hip.h: pcr_hip_sample_grid_host), one after the other.
inline void host_points(const Geom& g, const float* band, int64_t stride, const double* x, const double* y, const float* z,
                        uint64_t n, int mode, float* out) {
    if (mode == kBilinear) {
        if (z) host_loop<true, true>(g, band, stride, x, y, z, n, out);
        else host_loop<true, false>(g, band, stride, x, y, z, n, out);
    } else {
        if (z) host_loop<false, true>(g, band, stride, x, y, z, n, out);
        else host_loop<false, false>(g, band, stride, x, y, z, n, out);
    }
}

}  // namespace sample
}  // namespace pcrhip
