// points_in_polygons_san.cpp -- the index builder and the walk of the exact point-in-polygon test (csrc/point_in_polygon.hpp,
// csrc/point_in_polygon_index.hpp) under AddressSanitizer + UBSan, on the CPU: rectangles, a donut, a comb, overlapping n-gons,
// a partition with shared vertices, a triangle with a vertex far outside, polygons without a ring or without area -- each with the
// index forced to 1 x 1, 2 x 3, 7 x 5, 64 x 64 and automatic -- at every vertex, every edge's midpoint, one nextafter either side
// of those in x and in y, far outside, NaN and infinite coordinates.  The walk reads COPIES of the tables that are allocated
// exactly, as are the polygon and point arrays (no slack: ASan sees the first element outside any of them), and every answer is
// compared with the rule over all edges, no index.  Built and run by tests/test_points_in_polygons.py.
#include "point_in_polygon_index.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

namespace {

namespace pip = pcrhip::pip;
namespace rs = pcrhip::raster;

void fail(const char* what) {
    std::printf("FAILED: %s\n", what);
    std::exit(1);
}

struct Set {
    std::vector<double> coords;
    std::vector<int64_t> rings{0}, polys{0};
    void ring(const std::vector<double>& xy) {
        coords.insert(coords.end(), xy.begin(), xy.end());
        rings.push_back((int64_t)coords.size() / 2);
    }
    void end_polygon() { polys.push_back((int64_t)rings.size() - 1); }
};

std::vector<double> rect(double x0, double y0, double x1, double y1) { return {x0, y0, x1, y0, x1, y1, x0, y1}; }
std::vector<double> ngon(double cx, double cy, double r, int n, double phase) {
    std::vector<double> v;
    for (int i = 0; i < n; ++i) {
        const double a = phase + 2.0 * 3.14159265358979323846 * i / n;
        v.push_back(cx + r * std::cos(a));
        v.push_back(cy + r * std::sin(a));
    }
    return v;
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

uint32_t brute(const Set& s, double x, double y) {
    uint32_t won = 0;
    const int64_t P = (int64_t)s.polys.size() - 1;
    for (int64_t p = 0; p < P; ++p) {
        bool odd = false;
        for (int64_t j = s.polys[p]; j < s.polys[p + 1]; ++j) {
            const int64_t a0 = s.rings[j], n = s.rings[j + 1] - a0;
            for (int64_t i = 0; i < n; ++i) {
                const double* a = &s.coords[2 * (a0 + i)];
                const double* b = &s.coords[2 * (a0 + (i + 1 == n ? 0 : i + 1))];
                const bool up = a[1] <= b[1];
                const rs::Edge e{up ? a[1] : b[1], up ? b[1] : a[1], up ? a[0] : b[0], up ? b[0] : a[0]};
                if (rs::crosses(e, y) && rs::crossing_x(e, y) > x) odd = !odd;
            }
        }
        if (odd) won = (uint32_t)(p + 1);
    }
    return won;
}

size_t run(const Set& s, const char* what) {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int64_t V = (int64_t)s.coords.size() / 2, R = (int64_t)s.rings.size() - 1, P = (int64_t)s.polys.size() - 1;
    std::vector<double> xs, ys;
    auto around = [&](double x, double y) {
        const double dx[5] = {x, std::nextafter(x, -inf), std::nextafter(x, inf), x, x};
        const double dy[5] = {y, y, y, std::nextafter(y, -inf), std::nextafter(y, inf)};
        for (int k = 0; k < 5; ++k) xs.push_back(dx[k]), ys.push_back(dy[k]);
    };
    for (int64_t j = 0; j < R; ++j) {
        const int64_t a0 = s.rings[j], n = s.rings[j + 1] - a0;
        for (int64_t i = 0; i < n; ++i) {
            const double* a = &s.coords[2 * (a0 + i)];
            const double* b = &s.coords[2 * (a0 + (i + 1 == n ? 0 : i + 1))];
            around(a[0], a[1]);
            around((a[0] + b[0]) / 2, (a[1] + b[1]) / 2);
        }
    }
    const double special[] = {nan, inf, -inf, -1e300, 1e300, 0.0, 3.5};
    for (double x : special)
        for (double y : special) xs.push_back(x), ys.push_back(y);
    const size_t n = xs.size();
    const auto coords = exact(s.coords);
    const auto rings = exact(s.rings);
    const auto polys = exact(s.polys);
    const auto x = exact(xs), y = exact(ys);
    std::vector<uint32_t> want(n);
    for (size_t i = 0; i < n; ++i) want[i] = brute(s, xs[i], ys[i]);
    const int sizes[5][2] = {{1, 1}, {2, 3}, {7, 5}, {64, 64}, {0, 0}};
    for (const auto& size : sizes) {
        pip::BuildParams bp;
        bp.cols = size[0];
        bp.rows = size[1];
        pip::Index ix;
        std::string err;
        if (!pip::build_index(V ? coords.get() : nullptr, V, rings.get(), R, polys.get(), P, nullptr, bp, &ix, &err)) fail(err.c_str());
        const auto cell_start = exact(ix.cell_start);
        const auto items = exact(ix.items);
        const auto ey = exact(ix.ey);
        const auto ex = exact(ix.ex);
        if (ix.cell_start.size() != (size_t)ix.b.gx * (size_t)ix.b.gy + 1 || ix.cell_start.back() != ix.items.size()) fail("cell_start");
        for (const pip::Item& it : ix.items)
            if (it.count != pip::kInside && (uint64_t)it.start + it.count > ix.ey.size()) fail("an item names edges beyond the list");
        const pip::View v{ix.b, cell_start.get(), items.get(), ey.get(), ex.get(), nullptr, rs::kNanBits};
        for (size_t i = 0; i < n; ++i)
            if (pip::winner(v, x[i], y[i]) != want[i]) {
                std::printf("%s, index %d x %d, point %zu (%.17g, %.17g): %u, the rule says %u\n", what, size[0], size[1], i, x[i], y[i],
                            pip::winner(v, x[i], y[i]), want[i]);
                fail("the walk disagrees with the rule");
            }
        std::unique_ptr<float[]> out(new float[n]);              // the host loop itself, over threads
        pip::points_host(ix, x.get(), y.get(), n, out.get(), 3);
        for (size_t i = 0; i < n; ++i)
            if ((out[i] != out[i]) != (want[i] == 0u) || (want[i] && out[i] != (float)want[i])) fail("points_host");
    }
    return n;
}

}  // namespace

int main() {
    size_t points = 0;
    {
        Set s;
        s.ring(rect(2.0, 3.0, 40.0, 29.0)), s.end_polygon();
        s.ring(rect(10.0, 8.0, 20.0, 16.0)), s.end_polygon();
        s.ring(rect(40.0, 3.0, 64.0, 29.0)), s.end_polygon();
        points += run(s, "rectangles");
    }
    {
        Set s;
        s.ring(ngon(30, 30, 22, 24, 0.1)), s.ring(ngon(30, 30, 9, 24, 0.3)), s.end_polygon();
        points += run(s, "donut");
    }
    {
        Set s;                                                     // a comb of 9 teeth
        std::vector<double> c{1, 2, 28, 2, 28, 3.5};
        for (int i = 8; i >= 0; --i) {
            const double xa = 1 + 3.0 * i, xb = xa + 1.65;
            const double t[] = {xb, 3.5, xb, 8.5, xa, 8.5, xa, 3.5};
            c.insert(c.end(), t, t + 8);
        }
        s.ring(c), s.end_polygon();
        points += run(s, "comb");
    }
    {
        Set s;
        uint64_t seed = 12345;
        auto rnd = [&]() {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            return (double)(seed >> 11) * 0x1p-53;
        };
        for (int k = 0; k < 60; ++k) {
            const double cx = 200 * rnd(), cy = 150 * rnd(), r = 2 + 38 * rnd();
            s.ring(ngon(cx, cy, r, 3 + (int)(10 * rnd()), rnd())), s.end_polygon();
        }
        points += run(s, "overlapping n-gons");
    }
    {
        Set s;                                                     // 4 x 3 quadrilaterals over one jittered lattice of nodes
        double nx[4][5], ny[4][5];
        for (int j = 0; j < 4; ++j)
            for (int i = 0; i < 5; ++i) {
                nx[j][i] = 5 + 22.5 * i + ((i % 4) && (j % 3) ? 3.1 * ((i * 7 + j * 3) % 5 - 2) : 0.0);
                ny[j][i] = -7 + 22.7 * j + ((i % 4) && (j % 3) ? 2.3 * ((i * 5 + j * 11) % 5 - 2) : 0.0);
            }
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 4; ++i)
                s.ring({nx[j][i], ny[j][i], nx[j][i + 1], ny[j][i + 1], nx[j + 1][i + 1], ny[j + 1][i + 1], nx[j + 1][i], ny[j + 1][i]}), s.end_polygon();
        points += run(s, "partition");
    }
    {
        Set s;
        s.ring({0.0, 0.0, 10.0, 1.0, 1.0e7, 3.0e6}), s.end_polygon();
        s.ring(ngon(5.0, 0.6, 0.5, 5, 0.1)), s.end_polygon();
        points += run(s, "far triangle");
    }
    {
        Set s;
        s.ring(rect(0, 0, 8, 8)), s.end_polygon();
        s.end_polygon();                                           // no ring
        s.ring({1, 1, 3, 3, 5, 5}), s.end_polygon();               // no area
        s.ring({1, 2, 6, 2, 3, 2}), s.end_polygon();               // no edge that can cross
        s.ring(ngon(9, 9, 3, 7, 0.1)), s.end_polygon();
        points += run(s, "degenerate");
        Set none;
        points += run(none, "no polygon");
    }
    std::printf("builder and walk survived %zu points\n", points);
    return 0;
}
