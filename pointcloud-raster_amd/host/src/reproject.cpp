// reproject.cpp -- pcr/core/reproject.h, and the pieces of it the engines share (pipeline_common.h): CRS -> descriptor of the
// C-ABI, the host transform in chunks over OpenMP threads.  The per-point math is the C-ABI's (csrc/reproject.hpp), on the
// host through pcr_hip_transform_xy_host.
#include "pcr/core/reproject.h"

#include "buffer.h"
#include "pcr/core/point_cloud.h"
#include "pipeline_common.h"

#include <algorithm>
#include <cctype>
#include <cstdlib>

#ifdef _OPENMP
#include <omp.h>
#endif

namespace pcr {

namespace {

// EPSG code of an AUTHORITY["EPSG","n"] / ID["EPSG",n] node's argument list (text between its brackets), else 0
int epsg_of_args(const std::string& args) {
    size_t i = 0;
    auto skip = [&] { while (i < args.size() && std::isspace((unsigned char)args[i])) ++i; };
    auto token = [&]() -> std::string {                       // a quoted string ("" escapes a quote) or a bare word
        skip();
        std::string t;
        if (i < args.size() && args[i] == '"') {
            for (++i; i < args.size(); ++i) {
                if (args[i] == '"') {
                    if (i + 1 < args.size() && args[i + 1] == '"') { t += '"'; ++i; continue; }
                    ++i;
                    break;
                }
                t += args[i];
            }
        } else {
            while (i < args.size() && args[i] != ',' && !std::isspace((unsigned char)args[i])) t += args[i++];
        }
        skip();
        return t;
    };
    std::string auth = token();
    for (auto& ch : auth) ch = (char)std::toupper((unsigned char)ch);
    if (auth != "EPSG" || i >= args.size() || args[i] != ',') return 0;
    ++i;
    const std::string code = token();
    if (code.empty() || code.size() > 9 || !std::all_of(code.begin(), code.end(), [](char ch) { return std::isdigit((unsigned char)ch); }))
        return 0;
    return std::atoi(code.c_str());
}

// the top-level authority of a WKT1 / WKT2 string: the last AUTHORITY[...] or ID[...] that is a direct child of the outermost node
int wkt_epsg(const std::string& wkt) {
    int depth = 0, found = 0;
    size_t word_start = std::string::npos, args_start = 0;
    std::string child;                                        // keyword of the depth-1 node being read
    bool quoted = false;
    for (size_t i = 0; i < wkt.size(); ++i) {
        const char ch = wkt[i];
        if (quoted) {
            if (ch == '"') quoted = false;                    // ("" re-enters at once: the escape needs no special case)
            continue;
        }
        if (ch == '"') { quoted = true; continue; }
        if (std::isalnum((unsigned char)ch) || ch == '_') {
            if (word_start == std::string::npos) word_start = i;
            continue;
        }
        const std::string word = word_start == std::string::npos ? "" : wkt.substr(word_start, i - word_start);
        word_start = std::string::npos;
        if (ch == '[' || ch == '(') {
            if (depth == 1) {
                child = word;
                for (auto& c : child) c = (char)std::toupper((unsigned char)c);
                args_start = i + 1;
            }
            ++depth;
        } else if (ch == ']' || ch == ')') {
            --depth;
            if (depth == 1 && (child == "AUTHORITY" || child == "ID")) {
                const int code = epsg_of_args(wkt.substr(args_start, i - args_start));
                if (code) found = code;
            }
            if (depth == 1) child.clear();
            if (depth <= 0) break;                            // the outermost node is closed
        }
    }
    return found;
}

Status fail_crs(const std::string& msg) { return Status::error(StatusCode::CrsError, msg); }

}  // namespace

int crs_epsg(const CRS& crs) {
    if (crs.epsg != 0) return crs.epsg;
    return crs.wkt.empty() ? 0 : wkt_epsg(crs.wkt);
}

namespace detail {

Status crs_desc(const CRS& crs, const char* role, pcr_hip_crs_desc* out) {
    const int code = crs_epsg(crs);
    if (code == 0)
        return fail_crs(std::string("reproject: the ") + role + " CRS is unidentified (no EPSG code, and no top-level EPSG authority in its WKT)");
    if (pcr_hip_crs_from_epsg(code, out) != PCR_HIP_OK) return fail_crs(std::string("reproject: ") + pcr_hip_last_error());
    return Status::success();
}

Status transform_host(const pcr_hip_crs_desc& src, const pcr_hip_crs_desc& dst, const double* x, const double* y, double* ox,
                      double* oy, size_t n, int threads) {
    constexpr size_t kChunk = 1 << 16;
    const int64_t chunks = (int64_t)((n + kChunk - 1) / kChunk);
    int rc = PCR_HIP_OK;
#pragma omp parallel for num_threads(std::max(threads, 1)) schedule(static) reduction(max : rc)
    for (int64_t k = 0; k < chunks; ++k) {
        const size_t i0 = (size_t)k * kChunk, m = std::min(kChunk, n - i0);
        rc = std::max(rc, pcr_hip_transform_xy_host(&src, &dst, x + i0, y + i0, ox + i0, oy + i0, m));
    }
    if (rc != PCR_HIP_OK) return Status::error(static_cast<StatusCode>(rc), "reproject: the host transform failed");
    return Status::success();
}

}  // namespace detail

Status transform_xy(const CRS& src, const CRS& dst, const double* x, const double* y, double* ox, double* oy, size_t n,
                    MemoryLocation loc) {
    pcr_hip_crs_desc s, d;
    Status st = detail::crs_desc(src, "source", &s);
    if (!st.ok()) return st;
    if (!(st = detail::crs_desc(dst, "destination", &d)).ok()) return st;
    if (n == 0) return Status::success();
    if (loc != MemoryLocation::Device) {
        int threads = 1;
#ifdef _OPENMP
        threads = omp_get_max_threads();
#endif
        return detail::transform_host(s, d, x, y, ox, oy, n, threads);
    }
    if (!(st = detail::hip_status(pcr_hip_transform_xy(&s, &d, x, y, ox, oy, n, nullptr))).ok()) return st;
    return detail::hip_status(pcr_hip_stream_synchronize(nullptr));
}

Status reproject(PointCloud& cloud, const CRS& dst) {
    Status s = transform_xy(cloud.crs(), dst, cloud.x(), cloud.y(), cloud.x(), cloud.y(), cloud.count(), cloud.location());
    if (!s.ok()) return s;
    cloud.set_crs(dst);
    return Status::success();
}

}  // namespace pcr
