// overviews.h -- internal: the overview pyramid (pcr/io/grid_io.h: build_overviews) on the host, header-only so that the
// GeoTIFF writer needs no further object file, and on device bands for callers that hold them without a Grid around them
// (Pipeline::Impl::finalize; host/src/overviews.cpp).  The per-cell arithmetic is csrc/overview.hpp, the lines the HIP
// kernel compiles.
#pragma once

#include "../../csrc/overview.hpp"
#include "pcr/core/grid.h"
#include "pcr/core/types.h"

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

namespace pcr {
namespace detail {

namespace ov = pcrhip::overview;

/// 0 "average", 1 "nearest" (pcr_hip_downsample2's numbering), -1 anything else.
inline int overview_mode(const std::string& r) {
    if (r == "average") return ov::kAverage;
    if (r == "nearest") return ov::kNearest;
    return -1;
}

/// GeoTiffOptions::overviews -> a number of levels on a width x height image; -1: more than there are.
inline int overview_levels(int levels, int width, int height) {
    if (width <= 0 || height <= 0 || levels < -1) return -1;
    if (levels == -1) {                       // the reference: levels 2, 4, ... while min(W, H) / level >= 256
        int n = 0;
        for (int64_t f = 2; std::min(width, height) / f >= 256; f *= 2) ++n;
        return n;
    }
    return levels <= ov::max_levels(width, height) ? levels : -1;
}

// one level on the host: rows are independent, so the result does not depend on how they are shared out
inline void downsample_host(const float* src, int w, int h, float* dst, int mode) {
    const int w1 = ov::level_extent(w, 1), h1 = ov::level_extent(h, 1);
    const float out = ov::nodata();
#pragma omp parallel for schedule(static) if ((int64_t)w1 * h1 > 65536)
    for (int r = 0; r < h1; ++r) {
        const float* r0 = src + (int64_t)(2 * r) * w;
        const float* r1 = 2 * r + 1 < h ? r0 + w : nullptr;
        float* d = dst + (int64_t)r * w1;
        for (int c = 0; c < w1; ++c) {
            const bool right = 2 * c + 1 < w;
            d[c] = ov::down4(mode, r0[2 * c], right ? r0[2 * c + 1] : out, r1 ? r1[2 * c] : out,
                             r1 && right ? r1[2 * c + 1] : out);
        }
    }
}

/// `levels` (> 0, resolved) grids made from a host-resident grid, in its kind of host memory.
inline Status build_overviews_host(const Grid& grid, int levels, int mode, std::vector<std::unique_ptr<Grid>>& out) {
    out.clear();
    const int nb = grid.num_bands();
    std::vector<BandDesc> descs;
    for (int b = 0; b < nb; ++b) {
        descs.push_back(grid.band_desc(b));
        if (!grid.band_f32(b)) return Status::error(StatusCode::InvalidArgument, "overviews need Float32 bands");
    }
    for (int k = 1; k <= levels; ++k) {
        auto g = Grid::create(ov::level_extent(grid.cols(), k), ov::level_extent(grid.rows(), k), descs, grid.location());
        if (!g) { out.clear(); return Status::error(StatusCode::OutOfMemory, "build_overviews: failed to allocate level " + std::to_string(k)); }
        const Grid& from = k == 1 ? grid : *out.back();
        for (int b = 0; b < nb; ++b) downsample_host(from.band_f32(b), from.cols(), from.rows(), g->band_f32(b), mode);
        out.push_back(std::move(g));
    }
    return Status::success();
}

/// `levels` (> 0, resolved) Device grids made from the device bands d_bands[b] (width x height, dense), enqueued on
/// `stream`; nothing is synchronised.
Status build_overviews_device(const std::vector<const float*>& d_bands, int width, int height,
                              const std::vector<BandDesc>& descs, int levels, int mode, void* stream,
                              std::vector<std::unique_ptr<Grid>>& out);

}  // namespace detail
}  // namespace pcr
