// rasterize.hpp -- the arithmetic of polygon scan conversion (pcr_hip_rasterize_polygons, pcr::rasterize_polygons,
// Pipeline::set_zones(name, polygons)), for the device (csrc/rasterize.hip), the C-ABI's host twin and the host engine
// (host/src/polygons.cpp): all compile these lines, with contraction off, so a label grid burnt in HBM and one burnt by the host
// loop agree bit for bit.  The contract is written in include/pcr_hip.h ("polygons") and DESIGN.md section 25.
//
//   centre   cx(c) = min_x + (c + 0.5) * cell_size_x,  cy(r) = max_y + (r + 0.5) * cell_size_y: GridConfig::cell_to_world's own
//            expression (c + 0.5 is exact, then one rounded product and one rounded sum).  Each is monotone in its index, not
//            strictly so where a cell is smaller than the spacing of binary64 at the origin.
//   edge     endpoints ordered so that a.y <= b.y (equal y: horizontal, never crosses); it crosses row r when
//            a.y <= cy(r) < b.y; then t = (cy - a.y) / (b.y - a.y), xc = a.x + t * (b.x - a.x), each operation rounded once.
//   inside   cell (r, c) is inside a polygon when the number of its crossing edges of row r with xc > cx(c) is odd (all rings
//            together, even-odd).
//   span     what the kernel and the twin evaluate instead of the per-cell count.  For cell_size_x > 0 let k(xc) be the first
//            column with cx(k) >= xc (width if none): the crossing counts for exactly the columns below k.  Every ring is
//            closed, so a row has an even number of crossings, and "odd number of k above c" is "odd number of k at or below
//            c".  For cell_size_x < 0, k(xc) is the first column with cx(k) < xc and the crossing counts for the columns from
//            k on: the same "odd number of k at or below c".  k comes from an estimate that is then moved until the real
//            cx values on both sides of it say it is the first, so the span form is the per-cell rule bit for bit.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCR_RS_HD __host__ __device__ __forceinline__
#else
#define PCR_RS_HD inline
#endif

namespace pcrhip {
namespace raster {

constexpr int64_t kMaxPolygons = 2147483646LL;       // 2^31 - 2: index + 1 fits the uint32 plane with room for "none" = 0
constexpr double kMaxCoordinate = 1e100;             // |coordinate| above it is refused: no intermediate can overflow
constexpr uint32_t kNanBits = 0x7FC00000u;           // the default background

struct Geom {                                        // the fields of a grid the cell centres are made of
    double min_x, max_y, csx, csy;
    int w, h;
};

struct Edge {                                        // ordered: ay <= by; horizontal edges are not kept
    double ay, by, ax, bx;
};

PCR_RS_HD double cx(const Geom& g, int c) { return g.min_x + ((double)c + 0.5) * g.csx; }
PCR_RS_HD double cy(const Geom& g, int r) { return g.max_y + ((double)r + 0.5) * g.csy; }

PCR_RS_HD bool crosses(const Edge& e, double cyr) { return e.ay <= cyr && cyr < e.by; }
PCR_RS_HD double crossing_x(const Edge& e, double cyr) {
    const double t = (cyr - e.ay) / (e.by - e.ay);
    const double run = e.bx - e.ax;
    const double off = t * run;
    return e.ax + off;
}

// The first index i of [0, n] at which `past(i)` holds (n: nowhere), `past` being monotone false -> true; `est` is a guess.
// A few steps from the guess, then bisection: whatever the guess, the answer is the one the real comparisons give.
template <class Past>
PCR_RS_HD int first_past(int est, int n, Past past) {
    int k = est < 0 ? 0 : est > n ? n : est;
    for (int step = 0; step < 4; ++step) {
        if (k > 0 && past(k - 1)) --k;
        else if (k < n && !past(k)) ++k;
        else return k;
    }
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (past(mid)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// (v - origin) / cs - 0.5 as an index guess, any double (NaN, +-Inf included) into [0, n]
PCR_RS_HD int guess(double v, double origin, double cs, int n, bool up) {
    const double q = (v - origin) / cs - 0.5;
    const double e = up ? __builtin_ceil(q) : __builtin_floor(q) + 1.0;
    if (!(e > 0.0)) return 0;
    if (e >= (double)n) return n;
    return (int)e;
}

// k(x): cell_size_x > 0: the first column with cx(k) >= x; cell_size_x < 0: the first column with cx(k) < x.  In [0, w].
PCR_RS_HD int first_col(const Geom& g, double x) {
    if (g.csx > 0.0) return first_past(guess(x, g.min_x, g.csx, g.w, true), g.w, [&](int k) { return cx(g, k) >= x; });
    return first_past(guess(x, g.min_x, g.csx, g.w, false), g.w, [&](int k) { return cx(g, k) < x; });
}
// The same for rows and cy.  The rows with lo <= cy(r) < hi are [first_row(lo), first_row(hi)) for cell_size_y > 0 and
// [first_row(hi), first_row(lo)) for cell_size_y < 0.
PCR_RS_HD int first_row(const Geom& g, double y) {
    if (g.csy > 0.0) return first_past(guess(y, g.max_y, g.csy, g.h, true), g.h, [&](int k) { return cy(g, k) >= y; });
    return first_past(guess(y, g.max_y, g.csy, g.h, false), g.h, [&](int k) { return cy(g, k) < y; });
}
PCR_RS_HD void rows_between(const Geom& g, double lo, double hi, int& r0, int& r1) {
    if (g.csy > 0.0) {
        r0 = first_row(g, lo);
        r1 = first_row(g, hi);
    } else {
        r0 = first_row(g, hi);
        r1 = first_row(g, lo);
    }
}

// The columns k(xc) can take over a polygon whose vertices lie in [xmin, xmax]: xc is a.x + t * (b.x - a.x) with 0 <= t < 1
// in rounded operations, which stays between a.x and b.x up to 1.5 * 2^-52 * max(|a.x|, |b.x|); four times that is allowed for.
PCR_RS_HD void cols_between(const Geom& g, double xmin, double xmax, int& c0, int& c1) {
    const double ax = xmin < 0.0 ? -xmin : xmin, bx = xmax < 0.0 ? -xmax : xmax;
    const double slack = (ax > bx ? ax : bx) * 0x1p-50;
    const int a = first_col(g, xmin - slack), b = first_col(g, xmax + slack);
    c0 = a < b ? a : b;
    c1 = a < b ? b : a;
}

// The cells of one 64-column word that are inside: bit j of the result is the parity of `carry` and the bits 0 .. j of
// `toggles` (bit j set: a crossing has k == the word's column j).
PCR_RS_HD uint64_t inside_of(uint64_t toggles, bool carry) {
    uint64_t m = toggles;
    m ^= m << 1;
    m ^= m << 2;
    m ^= m << 4;
    m ^= m << 8;
    m ^= m << 16;
    m ^= m << 32;
    return carry ? ~m : m;
}

}  // namespace raster
}  // namespace pcrhip
