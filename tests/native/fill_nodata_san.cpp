// fill_nodata_san.cpp -- the host loop of fill_nodata (host/src/fill_nodata.h) under AddressSanitizer + UBSan, on the CPU:
// images smaller than the window (5 x 3 at R = 32, 1 x 1, one row, one column) with holes in all four corners, strided
// planes with guard cells, every radius on a ragged image, values that overflow the quotient's conversion to float.
// Built and run by tests/test_fill_nodata.py.
#include "fill_nodata.h"

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

// exactly w x h cells of src and dst are allocated (no slack: ASan sees the first cell outside either)
void run_dense(int w, int h, int R, const std::vector<float>& src, std::vector<float>& dst) {
    dst.assign((size_t)w * h, kGuard);
    pcr::detail::fill_nodata_host(src.data(), dst.data(), w, h, w, w, R);
    for (int i = 0; i < w * h; ++i)
        if (src[(size_t)i] == src[(size_t)i] && dst[(size_t)i] != src[(size_t)i]) fail("a valid cell changed");
}

}  // namespace

int main() {
    std::vector<float> dst;
    // holes in all four corners of a 5 x 3 image, R = 32: every window leaves the image on every side
    {
        const int w = 5, h = 3;
        std::vector<float> src((size_t)w * h);
        for (int i = 0; i < w * h; ++i) src[(size_t)i] = (float)(i + 1);
        src[0] = src[(size_t)w - 1] = src[(size_t)(h - 1) * w] = src[(size_t)h * w - 1] = kNaN;
        for (int R : {1, 2, 31, 32}) {
            run_dense(w, h, R, src, dst);
            for (int i = 0; i < w * h; ++i)
                if (!(dst[(size_t)i] == dst[(size_t)i])) fail("a corner hole with valid cells in range stayed NaN");
        }
    }
    // the smallest images; all NaN; one row; one column
    for (int R : {1, 32}) {
        std::vector<float> one(1, kNaN);
        run_dense(1, 1, R, one, dst);
        if (dst[0] == dst[0]) fail("1 x 1 NaN image");
        std::vector<float> row(40, 1.0f), col(40, 2.0f);
        row[0] = row[39] = row[20] = kNaN;
        col[0] = col[39] = kNaN;
        run_dense(40, 1, R, row, dst);
        run_dense(1, 40, R, col, dst);
        if (dst[0] != 2.0f || dst[39] != 2.0f) fail("1 x 40 column");
    }
    // every radius on a ragged image with every third cell a hole, values up to FLT_MAX and +-Inf: the quotient converts to
    // float out of range, sums become Inf and NaN
    {
        const int w = 37, h = 23;
        std::vector<float> src((size_t)w * h);
        for (int i = 0; i < w * h; ++i) {
            const int k = i % 11;
            src[(size_t)i] = i % 3 == 0 ? kNaN : k == 1 ? std::numeric_limits<float>::max() : k == 2 ? -std::numeric_limits<float>::max()
                           : k == 4 ? std::numeric_limits<float>::infinity() : k == 5 ? -std::numeric_limits<float>::infinity()
                           : k == 7 ? std::numeric_limits<float>::denorm_min() : (float)i * 0.37f;
        }
        for (int R = 1; R <= pcr::detail::fl::kMaxRadius; ++R) run_dense(w, h, R, src, dst);
    }
    // a window inside a strided plane: nothing outside the window's cells is read as a neighbour or written
    {
        const int w = 9, h = 7, ss = 13, ds = 11;
        std::vector<float> src((size_t)(h - 1) * ss + w, kNaN), out((size_t)(h - 1) * ds + w, kGuard);
        for (int r = 0; r < h; ++r)
            for (int c = 0; c < w; ++c) src[(size_t)r * ss + c] = (r + c) % 4 == 0 ? kNaN : 3.0f;
        pcr::detail::fill_nodata_host(src.data(), out.data(), w, h, ss, ds, 32);
        for (int r = 0; r < h; ++r) {
            for (int c = 0; c < w; ++c)
                if (out[(size_t)r * ds + c] != 3.0f) fail("strided window: every cell is 3 after the fill");
            for (int c = w; c < ds && r + 1 < h; ++c)
                if (out[(size_t)r * ds + c] != kGuard) fail("strided window: a store between the rows");
        }
    }
    std::printf("host fill survived\n");
    return 0;
}
