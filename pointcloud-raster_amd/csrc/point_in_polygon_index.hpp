// point_in_polygon_index.hpp -- (host only) the ONE builder of the point-in-polygon index and the host loop over points, for
// the C-ABI (csrc/point_in_polygon.hip) and for programs that compile it alone (tests/native/points_in_polygons_san.cpp).  No
// HIP in here.  The contract and the tables: point_in_polygon.hpp; why a cell without a local edge is uniform: DESIGN.md
// section 26.
//
// Per edge (horizontal ones included, for the classification only): the slack s = max(|ax|, |bx|) * 2^-50 (cols_between's bound
// on how far a crossing can leave the edge's x range), ix0 = bi(min - s), ix1 = bi(max + s), jy0 = bj(ay), jy1 = bj(by).  The
// edge is LOCAL to the cells [ix0, ix1] x [jy0, jy1].  A cell without a local edge of p is uniform for p: it gets an item only
// when p holds its representative, a point that bi and bj themselves map to the cell.  A cell with one is mixed: its item is a
// prefix of the (polygon, band) list of p's non-horizontal edges with jy0 <= j <= jy1, sorted by ix1 descending -- the edges
// with ix1 >= i, the only ones whose crossing can lie to the right of a point of column i.  Polygons are taken from the last to
// the first, so a cell's items come out in descending index order, and a cell that a polygon holds whole takes no further item.
#pragma once

#include "point_in_polygon.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace pcrhip {
namespace pip {

constexpr size_t kDefaultMaxBytes = (size_t)256 << 20;

struct BuildParams {
    uint32_t background = raster::kNanBits;
    int cols = 0, rows = 0;                          // 0: automatic
    size_t max_bytes = kDefaultMaxBytes;
};

struct Index {
    Bins b{0.0, 0.0, 0.0, 0.0, 1, 1};
    std::vector<uint32_t> cell_start;
    std::vector<Item> items;
    std::vector<EdgeY> ey;
    std::vector<EdgeX> ex;
    std::vector<float> values;
    bool has_values = false;
    uint32_t background = raster::kNanBits;
    int64_t polygons = 0;

    View view() const {
        return View{b, cell_start.data(), items.data(), ey.data(), ex.data(), has_values ? values.data() : nullptr, background};
    }
};

// ---- the tables in one block (what is uploaded): [cell_start][items][ey][ex][values], each piece on 256 bytes
struct Layout {
    size_t cell_start, items, ey, ex, values, total;
};
inline size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
inline Layout layout_of(size_t cells, size_t items, size_t listed, size_t values) {
    Layout l;
    l.cell_start = 0;
    l.items = padded((cells + 1) * 4);
    l.ey = l.items + padded(items * sizeof(Item));
    l.ex = l.ey + padded(listed * sizeof(EdgeY));
    l.values = l.ex + padded(listed * sizeof(EdgeX));
    l.total = l.values + padded(values * 4) + 256;   // (+ 256: the base is moved up to a multiple of 256)
    return l;
}
inline Layout layout_of(const Index& ix) {
    return layout_of((size_t)ix.b.gx * (size_t)ix.b.gy, ix.items.size(), ix.ey.size(), ix.has_values ? ix.values.size() : 0);
}

// ---- the refusals about the polygon arrays: pcr_hip_rasterize_polygons' own, message for message behind the prefix
inline bool offsets_ok(const int64_t* o, int64_t n, int64_t last) {
    if (!o || o[0] != 0 || o[n] != last) return false;
    for (int64_t i = 0; i < n; ++i)
        if (o[i] > o[i + 1]) return false;
    return true;
}
inline bool check_polygons(const double* coords, int64_t V, const int64_t* ring_offsets, int64_t R, const int64_t* polygon_offsets, int64_t P,
                           std::string* err) {
    auto no = [&](const char* m) {
        *err = m;
        return false;
    };
    if (!(coords || V == 0)) return no("null argument");
    if (!(V >= 0 && R >= 0 && P >= 0)) return no("a negative count");
    if (P > raster::kMaxPolygons) return no("more than 2^31 - 2 polygons");
    if (!(offsets_ok(ring_offsets, R, V) && offsets_ok(polygon_offsets, P, R))) return no("null or inconsistent offsets");
    for (int64_t j = 0; j < R; ++j)
        if (ring_offsets[j + 1] - ring_offsets[j] < 3) return no("a ring of fewer than 3 vertices");
    for (int64_t i = 0; i < 2 * V; ++i)
        if (!(std::fabs(coords[i]) <= raster::kMaxCoordinate)) return no("a coordinate is not finite or beyond 1e100");
    return true;
}

namespace detail {

struct BEdge {                                       // an edge with its bins
    double ay, by, ax, bx;
    int ix0, ix1, jy0, jy1;
};

// doubles in their order as unsigned integers, and back (finite values)
inline uint64_t key_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return (u >> 63) ? ~u : (u | ((uint64_t)1 << 63));
}
inline double of_key(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & ~((uint64_t)1 << 63)) : ~k;
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}

// A value of [lo, hi] that bin() maps to `i`: the middle of the nominal cell, or else the first double of [lo, hi] whose bin is
// at least i (bin is monotone).  false: no double of [lo, hi] maps to i.
inline bool representative(double lo, double hi, double origin, double inv, int g, int i, double* out) {
    if (inv > 0.0) {
        const double c = origin + ((double)i + 0.5) / inv;
        if (c >= lo && c <= hi && bin(c, origin, inv, g) == i) {
            *out = c;
            return true;
        }
    }
    uint64_t a = key_of(lo), b = key_of(hi);         // the first key in [a, b] with bin >= i
    if (bin(hi, origin, inv, g) < i) return false;
    while (a < b) {
        const uint64_t mid = a + (b - a) / 2;
        if (bin(of_key(mid), origin, inv, g) >= i) b = mid;
        else a = mid + 1;
    }
    *out = of_key(a);
    return bin(*out, origin, inv, g) == i;
}

enum { kBuilt = 0, kNoColumn, kNoRow, kOverCap, kRefused };

struct Rec {
    uint32_t cell;
    Item item;
};

inline int build_at(const double* coords, const int64_t* ring_offsets, const int64_t* polygon_offsets, int64_t P, double x0, double x1,
                    double y0, double y1, int gx, int gy, size_t max_bytes, Index* out, std::string* err) {
    Bins b{x0, y0, 0.0, 0.0, gx, gy};
    b.inv_x = (double)gx / (x1 - x0);
    b.inv_y = (double)gy / (y1 - y0);
    if (gx == 1 || !std::isfinite(b.inv_x)) b.inv_x = 0.0, b.gx = 1;     // (a box without width: one column)
    if (gy == 1 || !std::isfinite(b.inv_y)) b.inv_y = 0.0, b.gy = 1;
    gx = b.gx;
    gy = b.gy;
    std::vector<double> xr((size_t)gx), yr((size_t)gy);
    for (int i = 0; i < gx; ++i)
        if (!representative(x0, x1, b.x0, b.inv_x, gx, i, &xr[(size_t)i])) return kNoColumn;
    for (int j = 0; j < gy; ++j)
        if (!representative(y0, y1, b.y0, b.inv_y, gy, j, &yr[(size_t)j])) return kNoRow;

    const size_t cells = (size_t)gx * (size_t)gy;
    const size_t values = out->has_values ? (size_t)P : 0;
    if (layout_of(cells, 0, 0, values).total > max_bytes) return kOverCap;
    std::vector<uint8_t> closed(cells, 0);           // a later polygon holds the whole cell: nothing below it can win
    std::vector<Rec> recs;
    std::vector<EdgeY> ey;
    std::vector<EdgeX> ex;
    std::vector<BEdge> edges, band;
    std::vector<uint8_t> mixed;
    std::vector<size_t> band0;
    std::vector<int> ix1s;

    for (int64_t p = P - 1; p >= 0; --p) {
        edges.clear();
        size_t crossing_edges = 0;
        for (int64_t j = polygon_offsets[p]; j < polygon_offsets[p + 1]; ++j) {
            const int64_t a0 = ring_offsets[j], n = ring_offsets[j + 1] - a0;
            for (int64_t i = 0; i < n; ++i) {
                const double* a = coords + 2 * (a0 + i);
                const double* c = coords + 2 * (a0 + (i + 1 == n ? 0 : i + 1));          // closed implicitly
                const bool up = a[1] <= c[1];
                BEdge e{up ? a[1] : c[1], up ? c[1] : a[1], up ? a[0] : c[0], up ? c[0] : a[0], 0, 0, 0, 0};
                const double lo = std::min(e.ax, e.bx), hi = std::max(e.ax, e.bx);
                const double s = std::max(std::fabs(e.ax), std::fabs(e.bx)) * 0x1p-50;
                e.ix0 = bi(b, lo - s);
                e.ix1 = bi(b, hi + s);
                e.jy0 = bj(b, e.ay);
                e.jy1 = bj(b, e.by);
                edges.push_back(e);
                if (e.ay != e.by) ++crossing_edges;
            }
        }
        if (crossing_edges == 0) continue;           // no ring, or nothing that can cross: holds no point
        if (crossing_edges > ((size_t)1 << 30)) {
            *err = "a polygon of more than 2^30 edges";
            return kRefused;
        }
        int pi0 = gx, pi1 = -1, pj0 = gy, pj1 = -1;
        for (const BEdge& e : edges) {
            pi0 = std::min(pi0, e.ix0);
            pi1 = std::max(pi1, e.ix1);
            pj0 = std::min(pj0, e.jy0);
            pj1 = std::max(pj1, e.jy1);
        }
        const size_t bw = (size_t)(pi1 - pi0 + 1), bh = (size_t)(pj1 - pj0 + 1);
        mixed.assign(bw * bh, 0);
        band0.assign(bh + 1, 0);
        for (const BEdge& e : edges) {
            for (int j = e.jy0; j <= e.jy1; ++j)
                std::memset(mixed.data() + (size_t)(j - pj0) * bw + (size_t)(e.ix0 - pi0), 1, (size_t)(e.ix1 - e.ix0 + 1));
            if (e.ay != e.by)
                for (int j = e.jy0; j <= e.jy1; ++j) ++band0[(size_t)(j - pj0) + 1];
        }
        for (size_t j = 0; j < bh; ++j) band0[j + 1] += band0[j];
        const size_t listed0 = ey.size(), listed = band0[bh];
        if (layout_of(cells, recs.size(), listed0 + listed, values).total > max_bytes || listed0 + listed > 0x7FFFFFFFull) return kOverCap;
        band.resize(listed);
        {
            std::vector<size_t> at(band0.begin(), band0.end() - 1);
            for (const BEdge& e : edges)
                if (e.ay != e.by)
                    for (int j = e.jy0; j <= e.jy1; ++j) band[at[(size_t)(j - pj0)]++] = e;
        }
        ey.resize(listed0 + listed);
        ex.resize(listed0 + listed);
        for (size_t j = 0; j < bh; ++j) {
            BEdge* first = band.data() + band0[j];
            BEdge* last = band.data() + band0[j + 1];
            std::stable_sort(first, last, [](const BEdge& l, const BEdge& r) { return l.ix1 > r.ix1; });
            const size_t n = (size_t)(last - first);
            ix1s.resize(n);
            for (size_t k = 0; k < n; ++k) {
                ey[listed0 + band0[j] + k] = EdgeY{first[k].ay, first[k].by};
                ex[listed0 + band0[j] + k] = EdgeX{first[k].ax, first[k].bx};
                ix1s[k] = first[k].ix1;
            }
            const size_t start = listed0 + band0[j];
            const int row = pj0 + (int)j;
            size_t count = n;                        // the edges with ix1 >= i, i going up
            for (int i = pi0; i <= pi1; ++i) {
                while (count > 0 && ix1s[count - 1] < i) --count;
                const size_t cell = (size_t)row * (size_t)gx + (size_t)i;
                if (closed[cell] || count == 0) continue;
                if (mixed[j * bw + (size_t)(i - pi0)]) {
                    recs.push_back(Rec{(uint32_t)cell, Item{(uint32_t)(p + 1), (uint32_t)start, (uint32_t)count, 0u}});
                } else if (odd_crossings(ey.data() + start, ex.data() + start, (uint32_t)count, xr[(size_t)i], yr[(size_t)row])) {
                    recs.push_back(Rec{(uint32_t)cell, Item{(uint32_t)(p + 1), 0u, kInside, 0u}});
                    closed[cell] = 1;
                }
            }
            if (layout_of(cells, recs.size(), listed0 + listed, values).total > max_bytes || recs.size() > 0x7FFFFFFFull) return kOverCap;
        }
    }

    out->b = b;
    out->cell_start.assign(cells + 1, 0);
    for (const Rec& r : recs) ++out->cell_start[(size_t)r.cell + 1];
    for (size_t c = 0; c < cells; ++c) out->cell_start[c + 1] += out->cell_start[c];
    out->items.resize(recs.size());
    {
        std::vector<uint32_t> at(out->cell_start.begin(), out->cell_start.end() - 1);
        for (const Rec& r : recs) out->items[at[r.cell]++] = r.item;          // in the order made: polygon index descending
    }
    out->ey.swap(ey);
    out->ex.swap(ex);
    return kBuilt;
}

// The automatic side: about two cells per edge along each axis -- 2 * sqrt(edges), at least 1, at most kMaxIndexSide.
inline int auto_side(int64_t edges) {
    const double s = std::ceil(2.0 * std::sqrt((double)std::max<int64_t>(edges, 0)));
    return (int)std::min<double>(std::max(s, 1.0), (double)kMaxIndexSide);
}

}  // namespace detail

// Every refusal, then the tables.  false and *err (without a prefix) when refused.
inline bool build_index(const double* coords, int64_t V, const int64_t* ring_offsets, int64_t R, const int64_t* polygon_offsets, int64_t P,
                        const float* values, const BuildParams& params, Index* out, std::string* err) {
    if (!check_polygons(coords, V, ring_offsets, R, polygon_offsets, P, err)) return false;
    if (params.cols < 0 || params.cols > kMaxIndexSide || params.rows < 0 || params.rows > kMaxIndexSide) {
        *err = "index_cols and index_rows must be 0 (automatic) or 1 .. 2048";
        return false;
    }
    double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
    for (int64_t v = 0; v < V; ++v) {
        const double x = coords[2 * v], y = coords[2 * v + 1];
        x0 = v ? std::min(x0, x) : x;
        x1 = v ? std::max(x1, x) : x;
        y0 = v ? std::min(y0, y) : y;
        y1 = v ? std::max(y1, y) : y;
    }
    out->polygons = P;
    out->background = params.background;
    out->has_values = values != nullptr;
    if (values) out->values.assign(values, values + P);
    const int side = detail::auto_side(V);
    int gx = params.cols ? params.cols : side, gy = params.rows ? params.rows : side;
    const size_t cap = params.max_bytes ? params.max_bytes : kDefaultMaxBytes;
    for (;;) {
        const int rc = detail::build_at(coords, ring_offsets, polygon_offsets, P, x0, x1, y0, y1, gx, gy, cap, out, err);
        if (rc == detail::kBuilt) return true;
        if (rc == detail::kRefused) return false;
        if (rc == detail::kNoColumn && gx > 1) {
            gx = gx / 2;                              // a column narrower than binary64's spacing: no point can name it
            continue;
        }
        if (rc == detail::kNoRow && gy > 1) {
            gy = gy / 2;
            continue;
        }
        const bool can_x = !params.cols && gx > 1, can_y = !params.rows && gy > 1;
        if (rc == detail::kOverCap && (can_x || can_y)) {
            if (can_x) gx = gx / 2;
            if (can_y) gy = gy / 2;
            continue;
        }
        *err = (params.cols || params.rows) && (gx > 1 || gy > 1)
                   ? "the index tables exceed max_index_bytes at the index_cols and index_rows asked for"
                   : "the index tables exceed max_index_bytes";
        return false;
    }
}

// The host loop: every point independent, so the bits do not depend on how the points are shared out.
inline void points_host(const Index& ix, const double* x, const double* y, uint64_t n, float* out, int threads) {
    const View v = ix.view();
    auto run = [&](uint64_t i0, uint64_t i1) {
        for (uint64_t i = i0; i < i1; ++i) out[i] = value_of(v.values, v.background, winner(v, x[i], y[i]));
    };
    const uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), (n + 4095) / 4096));
    if (parts == 1) {
        run(0, n);
        return;
    }
    std::vector<std::thread> pool;
    for (uint64_t k = 0; k < parts; ++k) pool.emplace_back(run, n * k / parts, n * (k + 1) / parts);
    for (std::thread& t : pool) t.join();
}

}  // namespace pip
}  // namespace pcrhip
