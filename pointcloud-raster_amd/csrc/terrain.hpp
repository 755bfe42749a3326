// terrain.hpp -- the per-cell arithmetic of the terrain bands (slope, aspect, hillshade, TRI, TPI, roughness), for the device
// (csrc/terrain.hip) and the host (host/src/terrain.h): both compile these lines, so a band derived in HBM and one derived by
// the host loop agree bit for bit.
//
// The window.  a b c / d e f / g h i is the 3 x 3 window around cell e; row a b c is image row r - 1.  NaN is "no data";
// every NaN that leaves these functions is 0x7FC00000.  A neighbour outside the image or NaN is MISSING.
//   edges = 0 (gdaldem's default)          a cell with any missing neighbour is NaN
//   edges = 1 (gdaldem -compute_edges)     a missing neighbour takes e's value
//   e NaN                                  NaN in both modes
// Gradients (Horn's method, gdaldem's default), binary64, the additions in exactly this order, never an fma:
//   GX = ((c + 2f) + i) - ((a + 2d) + g)        p = GX * kx,  kx = z_factor / ( 8.0 * cell_size_x)
//   GY = ((a + 2b) + c) - ((g + 2h) + i)        q = GY * ky,  ky = z_factor / (-8.0 * cell_size_y)
//   s2 = p*p + q*q
// The cell sizes are signed: on a north-up grid (cell_size_y < 0) row r - 1 is north, q is dz/dNorth and p is dz/dEast; a
// south-up or west-going grid comes out right by the signs alone.
// Products, each Float32 and rounded once at the end (sqrt and / are the correctly rounded binary64 operations):
//   SlopeDegrees   atan_deg((float)sqrt(s2))
//   SlopePercent   (float)(100.0 * sqrt(s2))
//   Aspect         the compass bearing of the downslope direction (-p, -q) in [0, 360); -1.0f where p == 0 && q == 0.
//                  t = atan_deg((float)(|p| / |q|)); q <= 0: p > 0 ? 360 - t : t; q > 0: p > 0 ? 180 + t : 180 - t, in
//                  binary32; a 360 result is 0
//   Hillshade      L = (sin_alt - (p * ls + q * lc)) / sqrt(1.0 + s2); 1.0f when L <= 0, else (float)(1.0 + 254.0 * L):
//                  gdaldem's 1..255 scale.  sin_alt, ls = cos_alt * sin_az, lc = cos_alt * cos_az are binary64 constants the
//                  host computes once (pcr::terrain_light); the device never evaluates a sine
//   TRI            (float)((|a-e| + |b-e| + |c-e| + |d-e| + |f-e| + |g-e| + |h-e| + |i-e|) / 8.0), binary64, left to right
//   TPI            (float)(e - (a + b + c + d + f + g + h + i) / 8.0), binary64, left to right
//   Roughness      max9 - min9, one binary32 subtraction; max9 starts at a and takes b, c, ..., i in turn when v > max9, min9
//                  likewise with <  (so the sign of a zero is defined)
// +-Inf and denormals are ordinary values; a NaN they lead to (Inf - Inf) is 0x7FC00000 like every other.
// atan_deg is Cephes' atanf -- reduction at tan pi/8 and tan 3 pi/8, a 4-term odd polynomial -- times 180/pi, made of binary32
// multiplications, additions and divisions alone, each rounded: no fmaf, no libm, so a NumPy float32 restatement reproduces it.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCR_TERRAIN_HD __host__ __device__ __forceinline__
#else
#define PCR_TERRAIN_HD inline
#endif

namespace pcrhip {
namespace terrain {

// product ids: PCR_HIP_TERRAIN_* of include/pcr_hip.h, pcr::TerrainProduct
enum : int { kSlopeDegrees = 0, kSlopePercent = 1, kAspect = 2, kHillshade = 3, kTRI = 4, kTPI = 5, kRoughness = 6, kProducts = 7 };
constexpr unsigned kHornMask = 0x0Fu;          // the products made of p and q
constexpr unsigned kRuggedMask = 0x70u;        // the products made of the nine values themselves

// what a launch (a host loop) is given besides the band
struct Consts {
    double kx, ky;                   // scale()
    double sin_alt, ls, lc;          // pcr::terrain_light
};

PCR_TERRAIN_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

// kx (eight = 8.0) or ky (eight = -8.0) of a signed cell size; host only in practice, one division
PCR_TERRAIN_HD double scale(double z_factor, double eight, double cell_size) { return z_factor / (eight * cell_size); }

// atan(x) in degrees, x >= 0 (or NaN, which it returns)
PCR_TERRAIN_HD float atan_deg(float x) {
    float y, t;
    if (x > 2.414213562373095f) {            // tan 3 pi / 8
        y = 1.5707963267948966f;
        t = -(1.0f / x);
    } else if (x > 0.4142135623730950f) {    // tan pi / 8
        y = 0.7853981633974483f;
        t = (x - 1.0f) / (x + 1.0f);
    } else {
        y = 0.0f;
        t = x;
    }
    const float z = t * t;
    float u = 8.05374449538e-2f * z;
    u = u - 1.38776856032e-1f;
    u = u * z;
    u = u + 1.99777106478e-1f;
    u = u * z;
    u = u - 3.33329491539e-1f;
    u = u * z;
    u = u * t;
    u = u + t;
    y = y + u;
    return y * 57.29577951308232f;
}

// The window's missing neighbours dealt with (w = a..i in reading order); false: the cell is NaN in every product.
PCR_TERRAIN_HD bool window(float w[9], int edges) {
    const float e = w[4];
    bool ok = e == e;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 9; ++k) {
        if (k == 4 || w[k] == w[k]) continue;
        if (edges) w[k] = e;
        else ok = false;
    }
    return ok;
}

PCR_TERRAIN_HD float aspect(double p, double q) {
    if (p == 0.0 && q == 0.0) return -1.0f;
    const float t = atan_deg((float)(__builtin_fabs(p) / __builtin_fabs(q)));
    float r;
    if (q <= 0.0) r = p > 0.0 ? 360.0f - t : t;
    else r = p > 0.0 ? 180.0f + t : 180.0f - t;
    return r == 360.0f ? 0.0f : r;
}

PCR_TERRAIN_HD float hillshade(double p, double q, double s2, const Consts& k) {
    const double L = (k.sin_alt - (p * k.ls + q * k.lc)) / __builtin_sqrt(1.0 + s2);
    return L <= 0.0 ? 1.0f : (float)(1.0 + 254.0 * L);
}

// The products of `mask` (bit = product id) of a window that window() has seen, out[id]; `ok` is what window() answered.
// HORN / RUGGED: whether the instantiation can make the products of kHornMask / kRuggedMask at all.
template <bool HORN, bool RUGGED>
PCR_TERRAIN_HD void evaluate(const float w[9], bool ok, unsigned mask, const Consts& k, float out[kProducts]) {
    const double a = w[0], b = w[1], c = w[2], d = w[3], e = w[4], f = w[5], g = w[6], h = w[7], i = w[8];
    if (HORN && (mask & kHornMask)) {
        const double gx = ((c + 2.0 * f) + i) - ((a + 2.0 * d) + g);
        const double gy = ((a + 2.0 * b) + c) - ((g + 2.0 * h) + i);
        const double p = gx * k.kx, q = gy * k.ky;
        const double s2 = p * p + q * q;
        if (mask & (1u << kSlopeDegrees | 1u << kSlopePercent)) {
            const double s = __builtin_sqrt(s2);
            if (mask & (1u << kSlopeDegrees)) out[kSlopeDegrees] = atan_deg((float)s);
            if (mask & (1u << kSlopePercent)) out[kSlopePercent] = (float)(100.0 * s);
        }
        if (mask & (1u << kAspect)) out[kAspect] = aspect(p, q);
        if (mask & (1u << kHillshade)) out[kHillshade] = hillshade(p, q, s2, k);
    }
    if (RUGGED && (mask & (1u << kTRI))) {
        double s = __builtin_fabs(a - e) + __builtin_fabs(b - e);
        s = s + __builtin_fabs(c - e);
        s = s + __builtin_fabs(d - e);
        s = s + __builtin_fabs(f - e);
        s = s + __builtin_fabs(g - e);
        s = s + __builtin_fabs(h - e);
        s = s + __builtin_fabs(i - e);
        out[kTRI] = (float)(s / 8.0);
    }
    if (RUGGED && (mask & (1u << kTPI))) {
        double s = a + b;
        s = s + c;
        s = s + d;
        s = s + f;
        s = s + g;
        s = s + h;
        s = s + i;
        out[kTPI] = (float)(e - s / 8.0);
    }
    if (RUGGED && (mask & (1u << kRoughness))) {
        float hi = w[0], lo = w[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int n = 1; n < 9; ++n) {
            if (w[n] > hi) hi = w[n];
            if (w[n] < lo) lo = w[n];
        }
        out[kRoughness] = hi - lo;
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int n = 0; n < kProducts; ++n) {
        if (!(mask & (1u << n))) continue;
        out[n] = ok && out[n] == out[n] ? out[n] : nodata();
    }
}

}  // namespace terrain
}  // namespace pcrhip
