// ground_filter.h -- internal: ground_filter (pcr/core/ground_filter.h) on the host, header-only so that a program can drive it
// without the rest of the library, and what the pipelines need of it.  The contract and the window evaluation are
// csrc/ground_filter.hpp, the lines the HIP kernels compile.
#pragma once

#include "../../csrc/ground_filter.hpp"
#include "fill_nodata.h"
#include "pcr/core/grid.h"
#include "pcr/core/ground_filter.h"
#include "pcr/core/types.h"
#include "pcr/engine/pipeline.h"
#include "pipeline_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace pcr {
namespace detail {

namespace gf = pcrhip::ground;

// ---- the schedule ------------------------------------------------------------------------------------------------------------
/// "" when the spec is inside its ranges, else what is wrong with which field.
inline std::string ground_spec_error(const GroundFilterSpec& s) {
    if (s.max_radius_cells < 1 || s.max_radius_cells > gf::kMaxRadius) return "max_radius_cells must be between 1 and 64";
    if (!(s.slope >= 0.0f) || !std::isfinite(s.slope)) return "slope must be finite and not negative";
    if (!(s.initial_distance >= 0.0f) || !std::isfinite(s.initial_distance)) return "initial_distance must be finite and not negative";
    if (!(s.max_distance >= s.initial_distance) || !std::isfinite(s.max_distance))
        return "max_distance must be finite and not below initial_distance";
    return std::string();
}

/// The radii and thresholds of a spec that passed ground_spec_error, for a finite positive cell size.
inline void ground_levels(const GroundFilterSpec& s, double cell, std::vector<int>* radii, std::vector<float>* thresholds) {
    radii->clear();
    thresholds->clear();
    int prev = 0;
    for (int R = 1; R <= s.max_radius_cells; R = s.exponential ? 2 * R : R + 1) {
        double t = (double)s.initial_distance;
        if (prev) t = (double)s.initial_distance + (double)s.slope * cell * 2.0 * (double)(R - prev);
        radii->push_back(R);
        thresholds->push_back((float)std::min((double)s.max_distance, t));
        prev = R;
    }
}

// ---- the host loop -----------------------------------------------------------------------------------------------------------
// One window pass along the rows (COLS: along the columns) of a dense w x h plane, out != in.  Lines are independent and the
// minimum is exact: the bits do not depend on how the lines are shared out.
template <bool MAX, bool COLS>
inline void ground_pass_host(const float* in, float* out, int w, int h, int R) {
    constexpr int kBlock = 64;                                   // columns a column pass walks side by side
    const int lines = COLS ? (w + kBlock - 1) / kBlock : h;
#pragma omp parallel if ((int64_t)w * h > 4096)
    {
        std::vector<float> buf;
#pragma omp for schedule(dynamic, 4)
        for (int l = 0; l < lines; ++l) {
            if (!COLS) {
                buf.assign((size_t)w + 2 * R, gf::nodata());
                std::memcpy(buf.data() + R, in + (size_t)l * w, (size_t)w * sizeof(float));
                gf::line_window<MAX>(buf.data(), 1, R, w);
                std::memcpy(out + (size_t)l * w, buf.data(), (size_t)w * sizeof(float));
            } else {
                const int c0 = l * kBlock, n = std::min(kBlock, w - c0);
                buf.assign(((size_t)h + 2 * R) * kBlock, gf::nodata());
                for (int r = 0; r < h; ++r) std::memcpy(buf.data() + (size_t)(r + R) * kBlock, in + (size_t)r * w + c0, (size_t)n * sizeof(float));
                for (int j = 0; j < n; ++j) gf::line_window<MAX>(buf.data() + j, kBlock, R, h);
                for (int r = 0; r < h; ++r) std::memcpy(out + (size_t)r * w + c0, buf.data() + (size_t)r * kBlock, (size_t)n * sizeof(float));
            }
        }
    }
}

// One band on the host, dst != src, rows `src_stride` / `dst_stride` floats apart; the levels are valid (pcr_hip_ground_filter).
inline void ground_filter_host(const float* src, float* dst, int w, int h, int64_t src_stride, int64_t dst_stride, int levels,
                               const int* radii, const float* thresholds) {
    const size_t cells = (size_t)w * h;
    std::vector<float> a(cells), t1(cells), t2(cells);
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const float x = gf::clean(src[(int64_t)r * src_stride + c]);
            a[(size_t)r * w + c] = x;
            std::memcpy(dst + (int64_t)r * dst_stride + c, &x, sizeof(float));
        }
    const float out = gf::nodata();
    for (int k = 0; k < levels; ++k) {
        const int R = radii[k];
        ground_pass_host<false, false>(a.data(), t1.data(), w, h, R);
        ground_pass_host<false, true>(t1.data(), t2.data(), w, h, R);
        ground_pass_host<true, false>(t2.data(), t1.data(), w, h, R);
        ground_pass_host<true, true>(t1.data(), t2.data(), w, h, R);
#pragma omp parallel for schedule(static) if ((int64_t)w * h > 4096)
        for (int r = 0; r < h; ++r)
            for (int c = 0; c < w; ++c)
                if (gf::non_ground(a[(size_t)r * w + c], t2[(size_t)r * w + c], thresholds[k]))
                    std::memcpy(dst + (int64_t)r * dst_stride + c, &out, sizeof(float));
        a.swap(t2);
    }
}

inline void band_difference_host(const float* top, const float* gnd, float* dst, int w, int h, int64_t top_stride,
                                 int64_t gnd_stride, int64_t dst_stride) {
#pragma omp parallel for schedule(static) if ((int64_t)w * h > 4096)
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const float d = gf::difference(top[(int64_t)r * top_stride + c], gnd[(int64_t)r * gnd_stride + c]);
            std::memcpy(dst + (int64_t)r * dst_stride + c, &d, sizeof(float));
        }
}

// ---- PipelineConfig::ground ------------------------------------------------------------------------------------------------------
/// What a pipeline does about PipelineConfig::ground, decided at create.
struct GroundPlan {
    bool on = false;
    int source = -1, top = -1;           // indices of the output bands named (top < 0: no hag band)
    std::string dtm_name, hag_name;
    std::vector<int> radii;
    std::vector<float> thresholds;
    int extra_bands() const { return !on ? 0 : top >= 0 ? 2 : 1; }
};

inline Status plan_ground(const PipelineConfig& cfg, GroundPlan* plan) {
    *plan = GroundPlan();
    const auto& g = cfg.ground;
    if (g.source_band.empty()) return Status::success();
    auto refuse = [](const std::string& msg) { return Status::error(StatusCode::InvalidArgument, "pipeline: " + msg); };
    if (cfg.shard_row_begin >= 0 || cfg.shard_row_end >= 0)
        return refuse("ground filter needs the whole grid; filter the gathered grid with ground_filter");
    std::vector<std::string> names = output_band_names(cfg);
    auto index_of = [&names](const std::string& n) {
        const auto it = std::find(names.begin(), names.end(), n);
        return it == names.end() ? -1 : (int)(it - names.begin());
    };
    plan->source = index_of(g.source_band);
    if (plan->source < 0) return refuse("ground.source_band '" + g.source_band + "' names no output band");
    if (!g.top_band.empty()) {
        plan->top = index_of(g.top_band);
        if (plan->top < 0) return refuse("ground.top_band '" + g.top_band + "' names no output band");
    }
    if (g.dtm_band_name.empty() || index_of(g.dtm_band_name) >= 0)
        return refuse("ground.dtm_band_name '" + g.dtm_band_name + "' clashes with an output band");
    if (plan->top >= 0 && (g.hag_band_name.empty() || index_of(g.hag_band_name) >= 0 || g.hag_band_name == g.dtm_band_name))
        return refuse("ground.hag_band_name '" + g.hag_band_name + "' clashes with an output band");
    const std::string bad = ground_spec_error(g);
    if (!bad.empty()) return refuse("ground." + bad);
    const double cell = std::max(std::fabs(cfg.grid.cell_size_x), std::fabs(cfg.grid.cell_size_y));
    if (!(cell > 0.0) || !std::isfinite(cell)) return refuse("ground filter needs a finite, positive cell size");
    ground_levels(g, cell, &plan->radii, &plan->thresholds);
    plan->dtm_name = g.dtm_band_name;
    plan->hag_name = g.hag_band_name;
    plan->on = true;
    return Status::success();
}

/// The result grid's bands: the reductions', then the DTM, then the hag band if asked.
inline void append_ground_bands(const GroundPlan& plan, std::vector<BandDesc>& bands) {
    if (!plan.on) return;
    BandDesc b;
    b.dtype = DataType::Float32;
    b.is_state = false;
    b.name = plan.dtm_name;
    bands.push_back(b);
    if (plan.top < 0) return;
    b.name = plan.hag_name;
    bands.push_back(b);
}

/// What follows the finalized bands of a host-resident result whose ground bands (if any) are its last: the ground filter on
/// the RAW source band, fill_nodata (the DTM is filled like a Min band), then hag from the bands as they leave the pipeline.
/// more_bands: bands that follow the ground filter's and are none of this function's business (terrain.h).
inline Status finish_result_host(Grid& grid, std::vector<ReductionType> types, int fill_radius, const GroundPlan& plan,
                                 int more_bands = 0) {
    const int w = grid.cols(), h = grid.rows();
    const int dtm = (int)types.size();
    if (plan.on) {
        if (grid.num_bands() != dtm + plan.extra_bands() + more_bands || !grid.band_f32(plan.source) || !grid.band_f32(dtm))
            return Status::error(StatusCode::InvalidArgument, "pipeline: the result grid lacks the ground filter's bands");
        ground_filter_host(grid.band_f32(plan.source), grid.band_f32(dtm), w, h, w, w, (int)plan.radii.size(), plan.radii.data(),
                           plan.thresholds.data());
        types.push_back(ReductionType::Min);
    }
    Status s = fill_result_host(grid, types, fill_radius);
    if (!s.ok()) return s;
    if (plan.on && plan.top >= 0)
        band_difference_host(grid.band_f32(plan.top), grid.band_f32(dtm), grid.band_f32(dtm + 1), w, h, w, w, w);
    return Status::success();
}

}  // namespace detail
}  // namespace pcr
