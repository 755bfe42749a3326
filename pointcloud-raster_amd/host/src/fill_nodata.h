// fill_nodata.h -- internal: fill_nodata (pcr/core/fill_nodata.h) on the host, header-only so that a program can drive it
// without the rest of the library, and what the pipelines need of it.  The per-cell arithmetic is csrc/fill_nodata.hpp, the
// lines the HIP kernel compiles.
#pragma once

#include "../../csrc/fill_nodata.hpp"
#include "pcr/core/grid.h"
#include "pcr/core/types.h"

#include <cstring>
#include <vector>

namespace pcr {
namespace detail {

namespace fl = pcrhip::fill;

/// PipelineConfig::fill_nodata_radius fills the bands of these reductions: a NaN there means "unknown".  In a Sum or Count
/// band it means "no data here" and stays.
inline bool fills_nodata(ReductionType t) {
    return t == ReductionType::Average || t == ReductionType::WeightedAverage || t == ReductionType::Min ||
           t == ReductionType::Max || t == ReductionType::MostRecent;
}

// One band on the host, dst != src, rows `src_stride` / `dst_stride` floats apart.  Cells are independent: the bits do not
// depend on how the rows are shared out.
inline void fill_nodata_host(const float* src, float* dst, int w, int h, int64_t src_stride, int64_t dst_stride, int R) {
    std::vector<float> wt((size_t)(R + 1) * (R + 1), 0.0f);      // [|dr| * (R + 1) + |dc|], computed once per call
    std::vector<int> half((size_t)R + 1);
    for (int a = 0; a <= R; ++a) {
        half[(size_t)a] = fl::half_width(R, a);
        for (int b = 0; b <= R; ++b)
            if (a || b) wt[(size_t)a * (R + 1) + b] = fl::weight(a * a + b * b);
    }
#pragma omp parallel for schedule(dynamic, 4) if ((int64_t)w * h > 4096)
    for (int r = 0; r < h; ++r) {
        const float* srow = src + (int64_t)r * src_stride;
        float* drow = dst + (int64_t)r * dst_stride;
        std::memcpy(drow, srow, (size_t)w * sizeof(float));
        for (int c = 0; c < w; ++c) {
            if (srow[c] == srow[c]) continue;
            double s = 0.0, t = 0.0;
            const int dr0 = r - R < 0 ? -r : -R, dr1 = r + R >= h ? h - 1 - r : R;
            for (int dr = dr0; dr <= dr1; ++dr) {
                const int ar = dr < 0 ? -dr : dr, hw = half[(size_t)ar];
                const float* wrow = wt.data() + (size_t)ar * (R + 1);
                const float* nrow = src + (int64_t)(r + dr) * src_stride + c;
                const int dc0 = c - hw < 0 ? -c : -hw, dc1 = c + hw >= w ? w - 1 - c : hw;
                for (int dc = dc0; dc <= dc1; ++dc) {
                    const float x = nrow[dc];
                    if (x != x || (dr | dc) == 0) continue;
                    fl::accumulate(s, t, wrow[dc < 0 ? -dc : dc], x);
                }
            }
            const float f = fl::finish(s, t, srow[c]);
            std::memcpy(drow + c, &f, sizeof(float));
        }
    }
}

/// The bands of a host-resident result whose reduction fills_nodata, filled in place (through a copy of the band).
inline Status fill_result_host(Grid& grid, const std::vector<ReductionType>& types, int R) {
    if (R <= 0) return Status::success();
    const int w = grid.cols(), h = grid.rows();
    std::vector<float> raw;
    for (int b = 0; b < grid.num_bands() && b < (int)types.size(); ++b) {
        if (!fills_nodata(types[(size_t)b]) || !grid.band_f32(b)) continue;
        float* band = grid.band_f32(b);
        raw.assign(band, band + (size_t)w * h);
        fill_nodata_host(raw.data(), band, w, h, w, w, R);
    }
    return Status::success();
}

}  // namespace detail
}  // namespace pcr
