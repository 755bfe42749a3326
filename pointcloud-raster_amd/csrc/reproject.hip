// reproject.hip -- pcr_hip_crs_from_epsg / pcr_hip_transform_xy / pcr_hip_transform_xy_host (include/pcr_hip.h): the EPSG
// table, the device kernel and its host twin, both built from reproject.hpp.
#include "common.hpp"
#include "reproject.hpp"

#include <algorithm>
#include <cstring>

namespace pcrhip {
namespace {

constexpr int kBlock = 256;

// Krueger / Karney series coefficients from the third flattening n (Karney 2011, eqs. (35), (36) and the delta series of
// the conformal latitude), Horner in n; and the rectifying radius A = a / (1 + n) (1 + n^2/4 + n^4/64 + n^6/256).
void tm_series(pcr_hip_crs_desc* d) {
    const double n = d->f / (2.0 - d->f);
    auto poly = [n](std::initializer_list<double> c) {      // c[0] n + c[1] n^2 + ... (lowest power first)
        double r = 0.0;
        const double* p = c.begin();
        for (int i = (int)c.size() - 1; i >= 0; --i) r = (r + p[i]) * n;
        return r;
    };
    const double n2 = n * n;
    d->alpha[0] = poly({1.0 / 2, -2.0 / 3, 5.0 / 16, 41.0 / 180, -127.0 / 288, 7891.0 / 37800});
    d->alpha[1] = n * poly({13.0 / 48, -3.0 / 5, 557.0 / 1440, 281.0 / 630, -1983433.0 / 1935360});
    d->alpha[2] = n2 * poly({61.0 / 240, -103.0 / 140, 15061.0 / 26880, 167603.0 / 181440});
    d->alpha[3] = n2 * n * poly({49561.0 / 161280, -179.0 / 168, 6601661.0 / 7257600});
    d->alpha[4] = n2 * n2 * poly({34729.0 / 80640, -3418889.0 / 1995840});
    d->alpha[5] = n2 * n2 * n * poly({212378941.0 / 319334400});
    d->beta[0] = poly({1.0 / 2, -2.0 / 3, 37.0 / 96, -1.0 / 360, -81.0 / 512, 96199.0 / 604800});
    d->beta[1] = n * poly({1.0 / 48, 1.0 / 15, -437.0 / 1440, 46.0 / 105, -1118711.0 / 3870720});
    d->beta[2] = n2 * poly({17.0 / 480, -37.0 / 840, -209.0 / 4480, 5569.0 / 90720});
    d->beta[3] = n2 * n * poly({4397.0 / 161280, -11.0 / 504, -830251.0 / 7257600});
    d->beta[4] = n2 * n2 * poly({4583.0 / 161280, -108847.0 / 3991680});
    d->beta[5] = n2 * n2 * n * poly({20648693.0 / 638668800});
    d->delta[0] = poly({2.0, -2.0 / 3, -2.0, 116.0 / 45, 26.0 / 45, -2854.0 / 675});
    d->delta[1] = n * poly({7.0 / 3, -8.0 / 5, -227.0 / 45, 2704.0 / 315, 2323.0 / 945});
    d->delta[2] = n2 * poly({56.0 / 15, -136.0 / 35, -1262.0 / 105, 73814.0 / 2835});
    d->delta[3] = n2 * n * poly({4279.0 / 630, -332.0 / 35, -399572.0 / 14175});
    d->delta[4] = n2 * n2 * poly({4174.0 / 315, -144838.0 / 6237});
    d->delta[5] = n2 * n2 * n * poly({601676.0 / 22275});
    d->ka = d->k0 * d->a / (1.0 + n) * (1.0 + n2 * (1.0 / 4 + n2 * (1.0 / 64 + n2 / 256)));
}

constexpr double kA = 6378137.0;
constexpr double kInvfWgs84 = 298.257223563;
constexpr double kInvfGrs80 = 298.257222101;

void set_ellipsoid(pcr_hip_crs_desc* d, double invf) {
    d->a = kA;
    d->f = 1.0 / invf;
    d->e = std::sqrt(d->f * (2.0 - d->f));
}

void set_utm(pcr_hip_crs_desc* d, double invf, int zone, bool south) {
    d->kind = PCR_HIP_CRS_TRANSVERSE_MERCATOR;
    set_ellipsoid(d, invf);
    d->lon0 = -183.0 + 6.0 * zone;
    d->k0 = 0.9996;
    d->fe = 500000.0;
    d->fn = south ? 10000000.0 : 0.0;
    tm_series(d);
}

int check_desc(const pcr_hip_crs_desc* d, const char* what) {
    PCR_REQUIRE(d, std::string("transform_xy: null ") + what + " descriptor");
    PCR_REQUIRE(d->kind >= PCR_HIP_CRS_GEOGRAPHIC && d->kind <= PCR_HIP_CRS_TRANSVERSE_MERCATOR,
                std::string("transform_xy: ") + what + " descriptor of unknown kind");
    return PCR_HIP_OK;
}

// in place or disjoint (include/pcr_hip.h)
bool overlap_ok(const double* in, const double* out, uint64_t n) {
    return in == out || out + n <= in || in + n <= out;
}

template <int SK, int DK>
__global__ void __launch_bounds__(kBlock) k_transform_xy(pcr_hip_crs_desc src, pcr_hip_crs_desc dst, const double* x,
                                                         const double* y, double* ox, double* oy, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double px = __builtin_nontemporal_load(x + i), py = __builtin_nontemporal_load(y + i);
        double u, v;
        crs::transform_point(src, dst, SK, DK, px, py, &u, &v);
        __builtin_nontemporal_store(u, ox + i);
        __builtin_nontemporal_store(v, oy + i);
    }
}

template <int SK>
int launch_dst(const pcr_hip_crs_desc& s, const pcr_hip_crs_desc& d, const double* x, const double* y, double* ox, double* oy,
               uint64_t n, hipStream_t st) {
    // one point per lane: as many blocks as points need (the grid-stride loop only takes over beyond 2^30 blocks)
    const dim3 grid((unsigned)std::min<uint64_t>((n + kBlock - 1) / kBlock, (uint64_t)1 << 30)), block(kBlock);
    switch (d.kind) {
        case PCR_HIP_CRS_GEOGRAPHIC:
            hipLaunchKernelGGL((k_transform_xy<SK, PCR_HIP_CRS_GEOGRAPHIC>), grid, block, 0, st, s, d, x, y, ox, oy, n);
            break;
        case PCR_HIP_CRS_WEB_MERCATOR:
            hipLaunchKernelGGL((k_transform_xy<SK, PCR_HIP_CRS_WEB_MERCATOR>), grid, block, 0, st, s, d, x, y, ox, oy, n);
            break;
        default:
            hipLaunchKernelGGL((k_transform_xy<SK, PCR_HIP_CRS_TRANSVERSE_MERCATOR>), grid, block, 0, st, s, d, x, y, ox, oy, n);
            break;
    }
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" {

int pcr_hip_crs_from_epsg(int epsg, pcr_hip_crs_desc* out) {
    PCR_REQUIRE(out, "crs_from_epsg: null out pointer");
    pcr_hip_crs_desc d;
    std::memset(&d, 0, sizeof d);
    d.epsg = epsg;
    d.k0 = 1.0;
    if (epsg == 4326 || epsg == 4269 || epsg == 4258) {
        d.kind = PCR_HIP_CRS_GEOGRAPHIC;
        set_ellipsoid(&d, epsg == 4326 ? kInvfWgs84 : kInvfGrs80);
    } else if (epsg == 3857) {
        d.kind = PCR_HIP_CRS_WEB_MERCATOR;
        d.a = kA;
    } else if (epsg >= 32601 && epsg <= 32660) {
        set_utm(&d, kInvfWgs84, epsg - 32600, false);
    } else if (epsg >= 32701 && epsg <= 32760) {
        set_utm(&d, kInvfWgs84, epsg - 32700, true);
    } else if (epsg >= 26901 && epsg <= 26923) {
        set_utm(&d, kInvfGrs80, epsg - 26900, false);
    } else if (epsg >= 25828 && epsg <= 25838) {
        set_utm(&d, kInvfGrs80, epsg - 25800, false);
    } else {
        return fail(PCR_HIP_NOT_IMPLEMENTED,
                    "crs: EPSG:" + std::to_string(epsg) + " is not supported (supported: 4326, 4269, 4258, 3857, "
                    "32601-32660, 32701-32760, 26901-26923, 25828-25838)");
    }
    *out = d;
    return PCR_HIP_OK;
}

int pcr_hip_transform_xy(const pcr_hip_crs_desc* src, const pcr_hip_crs_desc* dst, const double* d_x, const double* d_y,
                         double* d_out_x, double* d_out_y, uint64_t n, pcr_hip_stream s) {
    int rc;
    if ((rc = check_desc(src, "source")) != PCR_HIP_OK || (rc = check_desc(dst, "destination")) != PCR_HIP_OK) return rc;
    if (n == 0) return PCR_HIP_OK;
    PCR_REQUIRE(d_x && d_y && d_out_x && d_out_y, "transform_xy: null array");
    PCR_REQUIRE(overlap_ok(d_x, d_out_x, n) && overlap_ok(d_y, d_out_y, n) && overlap_ok(d_x, d_out_y, n) &&
                overlap_ok(d_y, d_out_x, n) && d_out_x != d_out_y, "transform_xy: output arrays overlap the input partly");
    hipStream_t st = static_cast<hipStream_t>(s);
    if (src->epsg == dst->epsg && src->kind == dst->kind) {                  // the same CRS: bit for bit
        if (d_out_x != d_x) PCR_HIP_TRY(hipMemcpyAsync(d_out_x, d_x, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        if (d_out_y != d_y) PCR_HIP_TRY(hipMemcpyAsync(d_out_y, d_y, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        return PCR_HIP_OK;
    }
    switch (src->kind) {
        case PCR_HIP_CRS_GEOGRAPHIC: return launch_dst<PCR_HIP_CRS_GEOGRAPHIC>(*src, *dst, d_x, d_y, d_out_x, d_out_y, n, st);
        case PCR_HIP_CRS_WEB_MERCATOR: return launch_dst<PCR_HIP_CRS_WEB_MERCATOR>(*src, *dst, d_x, d_y, d_out_x, d_out_y, n, st);
        default: return launch_dst<PCR_HIP_CRS_TRANSVERSE_MERCATOR>(*src, *dst, d_x, d_y, d_out_x, d_out_y, n, st);
    }
}

int pcr_hip_transform_xy_host(const pcr_hip_crs_desc* src, const pcr_hip_crs_desc* dst, const double* h_x, const double* h_y,
                              double* h_out_x, double* h_out_y, uint64_t n) {
    int rc;
    if ((rc = check_desc(src, "source")) != PCR_HIP_OK || (rc = check_desc(dst, "destination")) != PCR_HIP_OK) return rc;
    if (n == 0) return PCR_HIP_OK;
    PCR_REQUIRE(h_x && h_y && h_out_x && h_out_y, "transform_xy: null array");
    PCR_REQUIRE(overlap_ok(h_x, h_out_x, n) && overlap_ok(h_y, h_out_y, n) && overlap_ok(h_x, h_out_y, n) &&
                overlap_ok(h_y, h_out_x, n) && h_out_x != h_out_y, "transform_xy: output arrays overlap the input partly");
    if (src->epsg == dst->epsg && src->kind == dst->kind) {
        if (h_out_x != h_x) std::memcpy(h_out_x, h_x, n * sizeof(double));
        if (h_out_y != h_y) std::memcpy(h_out_y, h_y, n * sizeof(double));
        return PCR_HIP_OK;
    }
    const pcr_hip_crs_desc s = *src, d = *dst;
    for (uint64_t i = 0; i < n; ++i) crs::transform_point(s, d, s.kind, d.kind, h_x[i], h_y[i], h_out_x + i, h_out_y + i);
    return PCR_HIP_OK;
}

}  // extern "C"
