// point_in_polygon.hpp -- the exact per-point point-in-polygon test (pcr_hip_points_in_polygons, pcr::points_in_polygons), for
// the device (csrc/point_in_polygon.hip), the C-ABI's host twin and the index builder (csrc/point_in_polygon_index.hpp): all
// compile these lines, with contraction off, so a channel made in HBM and one made by the host loop agree bit for bit.  The
// contract is written in include/pcr_hip.h ("polygon index") and DESIGN.md section 26.
//
//   rule     rasterize.hpp's, the cell centre replaced by the point (x, y): an edge, ordered a.y <= b.y, crosses the point's level
//            when a.y <= y < b.y (raster::crosses); then xc = raster::crossing_x(e, y); the point is inside polygon p when the
//            number of p's crossing edges with xc > x is odd, all rings together; the greatest polygon index wins.
//   special  every comparison with NaN is false: a NaN coordinate is in no polygon.  At x = -Inf all crossing edges count, an even
//            number; at x = +Inf none; at y = +-Inf nothing crosses.  Only NaN is short-cut (winner): the others take the walk.
//   index    an accelerator, never part of the contract: a uniform grid of gx * gy cells over the vertices' bounding box.  bin()
//            maps a coordinate to its column or row -- one rounded subtraction, one rounded product by a constant >= 0, so
//            MONOTONE non-decreasing in its argument; the builder classifies edges and the walk locates points with this same
//            function, and the builder's arguments live in index space (DESIGN.md section 26 has the constancy argument).
//            A cell's items are sorted by polygon index descending; an item either says "every point of this cell is inside p"
//            (count == kInside) or names a run of p's edges to count crossings over; the first polygon found to hold the point
//            is the answer and the walk stops.
#pragma once

#include "rasterize.hpp"

namespace pcrhip {
namespace pip {

constexpr uint32_t kInside = 0xFFFFFFFFu;            // Item::count: no edges, the whole cell is inside
constexpr int kMaxIndexSide = 2048;

struct Item {
    uint32_t poly;                                   // polygon index + 1
    uint32_t start;                                  // into the listed edges
    uint32_t count;                                  // edges to test, or kInside
    uint32_t pad_;
};
struct EdgeY {
    double ay, by;
};
struct EdgeX {
    double ax, bx;
};
static_assert(sizeof(Item) == 16 && sizeof(EdgeY) == 16 && sizeof(EdgeX) == 16, "index table layout");

struct Bins {
    double x0, y0, inv_x, inv_y;                     // inv: cells per unit, >= 0 (0: a single cell)
    int gx, gy;
};

// The column (or row) of v: q = (v - origin) * inv; q <= 0 or NaN -> 0, q >= g -> g - 1, else floor(q).
PCR_RS_HD int bin(double v, double origin, double inv, int g) {
    const double d = v - origin;
    const double q = d * inv;
    if (!(q > 0.0)) return 0;
    if (q >= (double)g) return g - 1;
    return (int)q;                                   // (0 < q < g: truncation is floor)
}
PCR_RS_HD int bi(const Bins& b, double x) { return bin(x, b.x0, b.inv_x, b.gx); }
PCR_RS_HD int bj(const Bins& b, double y) { return bin(y, b.y0, b.inv_y, b.gy); }

struct View {                                        // the tables, where they are read
    Bins b;
    const uint32_t* cell_start;                      // [gx * gy + 1] into items
    const Item* items;
    const EdgeY* ey;
    const EdgeX* ex;
    const float* values;                             // null: (float)(p + 1)
    uint32_t background;
};

// The parity of the crossings to the right of (x, y) among n edges: the rule itself.
PCR_RS_HD bool odd_crossings(const EdgeY* ey, const EdgeX* ex, uint32_t n, double x, double y) {
    bool odd = false;
    for (uint32_t e = 0; e < n; ++e) {
        if (!(ey[e].ay <= y && y < ey[e].by)) continue;
        const raster::Edge ed{ey[e].ay, ey[e].by, ex[e].ax, ex[e].bx};
        if (raster::crossing_x(ed, y) > x) odd = !odd;
    }
    return odd;
}

// The winning polygon's index + 1 at (x, y), 0 where no polygon holds the point: the walk of the point's cell.
PCR_RS_HD uint32_t winner(const View& v, double x, double y) {
    if (x != x || y != y) return 0u;
    const int64_t cell = (int64_t)bj(v.b, y) * v.b.gx + bi(v.b, x);
    for (uint32_t it = v.cell_start[cell]; it < v.cell_start[cell + 1]; ++it) {
        const Item item = v.items[it];
        if (item.count == kInside) return item.poly;
        if (odd_crossings(v.ey + item.start, v.ex + item.start, item.count, x, y)) return item.poly;
    }
    return 0u;
}

PCR_RS_HD float value_of(const float* values, uint32_t background, uint32_t poly) {
    union {
        uint32_t u;
        float f;
    } bg;
    bg.u = background;
    if (poly == 0u) return bg.f;
    return values ? values[poly - 1u] : (float)poly;
}

}  // namespace pip
}  // namespace pcrhip
