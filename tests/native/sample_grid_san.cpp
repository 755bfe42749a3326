// sample_grid_san.cpp -- the host loop of sample_grid (csrc/sample_grid.hpp) under AddressSanitizer + UBSan, on the CPU: the
// lattice of tests/test_sample_grid.py -- cell centres, edges and corners, the bounds and one ulp either side of them, points
// far outside, NaN and infinite coordinates -- over surfaces of 1 x 1, 1 x 5, 5 x 1, 2 x 2 and 33 x 65 cells, north-up and
// south-up, dense and as a window of a larger plane, both modes, with and without a value channel, in place.  The band and
// the point arrays are allocated exactly (no slack: ASan sees the first element outside any of them).
// Built and run by tests/test_sample_grid.py.
#include "sample_grid.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

namespace {

namespace sg = pcrhip::sample;

const float kNaN = std::numeric_limits<float>::quiet_NaN();
const float kInf = std::numeric_limits<float>::infinity();
const float kGuard = -12345.5f;

void fail(const char* what) {
    std::printf("FAILED: %s\n", what);
    std::exit(1);
}

std::vector<double> axis(double origin, double cs, int n, double lo, double hi) {
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> v;
    for (int k = 0; k <= n; ++k) {
        const double edge = origin + k * cs;
        v.push_back(edge);
        v.push_back(std::nextafter(edge, -inf));
        v.push_back(std::nextafter(edge, inf));
        if (k < n) {
            const double c = origin + (k + 0.5) * cs;
            v.push_back(c);
            v.push_back(std::nextafter(c, -inf));
            v.push_back(std::nextafter(c, inf));
            v.push_back(origin + (k + 0.25) * cs);
        }
    }
    for (double b : {lo, hi}) {
        v.push_back(b);
        v.push_back(std::nextafter(b, -inf));
        v.push_back(std::nextafter(b, inf));
    }
    v.push_back(lo - 1e300);
    v.push_back(hi + 1e300);
    v.push_back(inf);
    v.push_back(-inf);
    v.push_back(std::numeric_limits<double>::quiet_NaN());
    return v;
}

void run(int w, int h, double csx, double csy, int64_t stride) {
    sg::Geom g;
    g.min_x = -37.5; g.max_y = 12.0;
    g.max_x = g.min_x + w * std::fabs(csx);
    g.min_y = g.max_y - h * std::fabs(csy);
    g.csx = csx; g.csy = csy; g.W = w; g.H = h;
    std::vector<float> band((size_t)((h - 1) * stride + w), kGuard);
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const int k = (r * w + c) % 7;
            band[(size_t)(r * stride + c)] = k == 3 ? kNaN : k == 5 ? kInf : k == 6 ? -kInf : (float)(r * 3 - c) * 0.37f;
        }
    const std::vector<double> ax = axis(g.min_x, csx, w, g.min_x, g.max_x), ay = axis(g.max_y, csy, h, g.min_y, g.max_y);
    std::vector<double> x, y;
    for (size_t j = 0; j < ay.size(); j += (ay.size() > 150 ? 3 : 1))
        for (size_t i = 0; i < ax.size(); ++i) { x.push_back(ax[i]); y.push_back(ay[j]); }
    const size_t n = x.size();
    std::vector<float> z(n), out(n), inplace(n);
    for (size_t i = 0; i < n; ++i) z[i] = i % 13 == 0 ? kNaN : i % 17 == 0 ? kInf : (float)(i % 101) * 0.5f;
    for (int mode : {sg::kNearest, sg::kBilinear}) {
        for (int with_value = 0; with_value < 2; ++with_value) {
            out.assign(n, kGuard);
            sg::host_points(g, band.data(), stride, x.data(), y.data(), with_value ? z.data() : nullptr, (uint64_t)n, mode, out.data());
            for (size_t i = 0; i < n; ++i) {
                uint32_t bits;
                __builtin_memcpy(&bits, &out[i], 4);
                if (out[i] != out[i] && bits != 0x7FC00000u) fail("a NaN that is not 0x7FC00000");
                if (out[i] == kGuard && !with_value) fail("a guard cell between the rows was read, or an output not stored");
                const bool inside = x[i] >= g.min_x && x[i] <= g.max_x && y[i] >= g.min_y && y[i] <= g.max_y;
                if (!inside && out[i] == out[i]) fail("a point outside the bounds sampled a value");
            }
            if (with_value) {
                inplace = z;
                sg::host_points(g, band.data(), stride, x.data(), y.data(), inplace.data(), (uint64_t)n, mode, inplace.data());
                if (__builtin_memcmp(inplace.data(), out.data(), n * sizeof(float)) != 0) fail("in place differs from out of place");
            }
        }
    }
    sg::host_points(g, band.data(), stride, nullptr, nullptr, nullptr, 0, sg::kBilinear, nullptr);      // n == 0 touches nothing
}

}  // namespace

int main() {
    const int shapes[5][2] = {{1, 1}, {1, 5}, {5, 1}, {2, 2}, {33, 65}};
    for (const auto& s : shapes) {
        run(s[0], s[1], 1.5, -0.75, s[0]);           // north-up, dense
        run(s[0], s[1], 0.5, 2.0, s[0]);             // south-up: every row clamps to 0
        run(s[0], s[1], 1.5, -0.75, s[0] + 5);       // a window of a wider plane: the guard cells between the rows are never sampled
        run(s[0], s[1], 1e-300, -1e300, s[0]);       // degenerate cell sizes: quotients far beyond an int, and tiny
    }
    std::printf("host loop survived\n");
    return 0;
}
