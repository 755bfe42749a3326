// ground_filter_san.cpp -- the host loop of the ground filter (host/src/ground_filter.h) under AddressSanitizer + UBSan, on
// the CPU: images smaller than the window (1 x 1, one row, one column, 7 x 5 at R = 64), ragged images through whole
// schedules, strided planes with guard cells, values whose differences overflow.  Built and run by tests/test_ground_filter.py.
#include "ground_filter.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

namespace {

const float kNaN = std::numeric_limits<float>::quiet_NaN();
const float kGuard = -12345.5f;

void fail(const char* what) {
    std::printf("FAILED: %s\n", what);
    std::exit(1);
}

std::vector<float> scene(int w, int h, int nan_every) {
    std::vector<float> a((size_t)w * h);
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const int i = r * w + c, k = i % 13;
            float v = 10.0f + 0.01f * (float)c + 0.02f * (float)r;
            if (r % 17 > 11 && c % 19 > 12) v += 5.0f;                                  // boxes
            if (k == 3) v = std::numeric_limits<float>::max();
            if (k == 5) v = -std::numeric_limits<float>::max();
            if (k == 7) v = std::numeric_limits<float>::infinity();
            if (k == 9) v = -std::numeric_limits<float>::infinity();
            if (k == 11) v = std::numeric_limits<float>::denorm_min();
            if (nan_every == 1 || (nan_every > 1 && i % nan_every == 0)) v = kNaN;
            a[(size_t)i] = v;
        }
    return a;
}

// exactly w x h cells of src and dst are allocated (no slack: ASan sees the first cell outside either)
void run_dense(int w, int h, const pcr::GroundFilterSpec& spec, const std::vector<float>& src) {
    std::vector<int> radii;
    std::vector<float> thresholds;
    pcr::detail::ground_levels(spec, 1.0, &radii, &thresholds);
    std::vector<float> dst((size_t)w * h, kGuard);
    pcr::detail::ground_filter_host(src.data(), dst.data(), w, h, w, w, (int)radii.size(), radii.data(), thresholds.data());
    for (int i = 0; i < w * h; ++i) {
        const float s = src[(size_t)i], d = dst[(size_t)i];
        if (d == kGuard) fail("a cell of dst was not stored");
        if (d == d && std::memcmp(&d, &s, 4) != 0) fail("a ground cell does not hold its source bits");
        if (s != s && d == d) fail("an empty cell became ground");
    }
    std::vector<float> hag((size_t)w * h, kGuard);
    pcr::detail::band_difference_host(src.data(), dst.data(), hag.data(), w, h, w, w, w);
    for (int i = 0; i < w * h; ++i)
        if (hag[(size_t)i] == kGuard) fail("a cell of hag was not stored");
}

}  // namespace

int main() {
    const int shapes[6][2] = {{1, 1}, {1, 40}, {40, 1}, {7, 5}, {45, 67}, {70, 130}};       // rows, cols
    for (const auto& sh : shapes)
        for (int nan_every : {0, 5, 1}) {
            const std::vector<float> src = scene(sh[1], sh[0], nan_every);
            for (int max_radius : {1, 3, 16, 64})
                for (bool exponential : {true, false}) {
                    if (!exponential && max_radius == 64 && sh[0] * sh[1] > 100) continue;   // (64 levels on the larger images: minutes under ASan)
                    pcr::GroundFilterSpec spec;
                    spec.max_radius_cells = max_radius;
                    spec.exponential = exponential;
                    run_dense(sh[1], sh[0], spec, src);
                }
        }
    // a window inside strided planes: nothing outside the window's cells is read as a neighbour or written
    {
        const int w = 9, h = 7, ss = 13, ds = 11;
        std::vector<float> src((size_t)(h - 1) * ss + w, -1000.0f), out((size_t)(h - 1) * ds + w, kGuard);
        for (int r = 0; r < h; ++r)
            for (int c = 0; c < w; ++c) src[(size_t)r * ss + c] = r == 3 && c == 4 ? 9.0f : 3.0f;
        const int radii[2] = {1, 64};
        const float thresholds[2] = {0.5f, 0.5f};
        pcr::detail::ground_filter_host(src.data(), out.data(), w, h, ss, ds, 2, radii, thresholds);
        for (int r = 0; r < h; ++r) {
            for (int c = 0; c < w; ++c) {
                const float d = out[(size_t)r * ds + c];
                if (r == 3 && c == 4 ? d == d : d != 3.0f) fail("strided window: the spike goes, the plain stays (a -1000 between the rows would take it all)");
            }
            for (int c = w; c < ds && r + 1 < h; ++c)
                if (out[(size_t)r * ds + c] != kGuard) fail("strided window: a store between the rows");
        }
    }
    std::printf("host ground filter survived\n");
    return 0;
}
