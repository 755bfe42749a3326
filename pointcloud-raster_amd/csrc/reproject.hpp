// reproject.hpp -- the coordinate transform of pcr_hip_transform_xy[_host], one point at a time.  __host__ __device__:
// reproject.hip compiles it into the gfx950 kernel and, for the host engine, into pcr_hip_transform_xy_host -- one source
// for both engines.
//
// Every transform goes source -> geographic -> destination.  The geographic intermediate is (longitude in degrees,
// latitude in radians, sin and cos of the latitude); each stage takes what it needs and derives the rest without a second
// transcendental call where an identity gives it.  Transverse Mercator is Krueger's series to n^6 in the form of
// C. F. F. Karney, "Transverse Mercator with an accuracy of a few nanometers", J. Geodesy 85 (2011) 475-485: forward
// eqs. (7)-(11) with the alpha series, inverse with the beta series and the conformal -> geodetic latitude series (delta),
// both evaluated by Clenshaw summation on the complex argument.  f64 throughout; out-of-domain points (kTmEtaMax below for
// Transverse Mercator) and non-finite input become NaN on both axes.
#pragma once

#include <cmath>

#include "pcr_hip.h"

#if defined(__HIPCC__)
#define PCR_HD __host__ __device__
#else
#define PCR_HD
#endif

namespace pcrhip {
namespace crs {

constexpr double kPi = 3.14159265358979323846;
constexpr double kD2R = kPi / 180.0;
constexpr double kR2D = 180.0 / kPi;

// Transverse Mercator is accepted where |eta'| <= kTmEtaMax, eta' = atanh(cos chi sin(lambda - lambda0)) the Gauss-Schreiber
// easting (chi the conformal latitude): the n^7 term the series drops grows like sinh(14 eta'), and at this cut the host
// form is within 2.5e-7 m of the exact map.  About 50 degrees from the central meridian on the equator, any
// |lambda - lambda0| < 90 near the poles.  The forward direction tests z = sinh(eta'), the inverse the beta-corrected eta'.
constexpr double kTmEtaMax = 1.0;
constexpr double kTmSinhEtaMax = 1.1752011936438014;     // sinh(kTmEtaMax)

// longitude difference in degrees -> (-180, 180]
PCR_HD inline double norm_deg(double d) {
    if (d > -180.0 && d <= 180.0) return d;
    d = fmod(d, 360.0);                     // (-360, 360)
    if (d > 180.0) d -= 360.0;
    else if (d <= -180.0) d += 360.0;
    return d;
}

struct Geo {
    double lon;        // degrees, as the source gave it or (-180, 180] when computed
    double phi;        // radians (only when the destination is geographic: see decode)
    double s, c;       // sin, cos of the latitude
};

// sum_{j=1..6} a_j sin(2 j z), z = xi + i eta, given sin/cos(2 xi) and sinh/cosh(2 eta): Clenshaw on the complex argument
PCR_HD inline void clenshaw_sin(const double* a, double s2x, double c2x, double sh2y, double ch2y, double* re, double* im) {
    const double ar = 2.0 * c2x * ch2y, ai = -2.0 * s2x * sh2y;            // 2 cos(2z)
    double br = 0.0, bi = 0.0, cr = 0.0, ci = 0.0;                          // b_{k+1}, b_{k+2}
    for (int k = 5; k >= 0; --k) {
        const double tr = a[k] + (ar * br - ai * bi) - cr;
        const double ti = (ar * bi + ai * br) - ci;
        cr = br; ci = bi;
        br = tr; bi = ti;
    }
    const double sr = s2x * ch2y, si = c2x * sh2y;                          // sin(2z)
    *re = sr * br - si * bi;
    *im = sr * bi + si * br;
}

// sinh and cosh of sigma = e atanh(e sin phi) by their series: |e sin phi| <= e = 0.082 and |sigma| <= 0.0068, so atanh to
// z^17 and sinh / cosh to sigma^7 / sigma^6 are exact in f64 (the first dropped terms are below 1e-18 relative) -- no log,
// no exp, no division
PCR_HD inline void sinh_cosh_sigma(double e, double sphi, double* sh, double* ch) {
    const double z = e * sphi, w = z * z;
    double p = 1.0 / 17;
    p = p * w + 1.0 / 15; p = p * w + 1.0 / 13; p = p * w + 1.0 / 11; p = p * w + 1.0 / 9;
    p = p * w + 1.0 / 7;  p = p * w + 1.0 / 5;  p = p * w + 1.0 / 3;  p = p * w + 1.0;
    const double sg = e * (z * p), s2 = sg * sg;
    *sh = sg + sg * (s2 * (1.0 / 6 + s2 * (1.0 / 120 + s2 * (1.0 / 5040))));
    *ch = 1.0 + s2 * (1.0 / 2 + s2 * (1.0 / 24 + s2 * (1.0 / 720)));
}

// sinh and cosh from one expm1 (exact near 0, where exp(x) - exp(-x) would cancel)
PCR_HD inline void sinh_cosh(double x, double* sh, double* ch) {
    const double m = expm1(x), ip = 1.0 / (1.0 + m);                     // exp(x) - 1, exp(-x)
    *sh = 0.5 * (m + m * ip);
    *ch = 0.5 * ((1.0 + m) + ip);
}

// ---- source -> geographic ------------------------------------------------------------------------------------------------
// false: outside the source's domain (the point becomes NaN)
// kind == d.kind, passed apart so that a kernel instantiated per (source, destination) kind folds the switch away
PCR_HD inline bool decode(const pcr_hip_crs_desc& d, int kind, double x, double y, bool need_phi, Geo* g) {
    switch (kind) {
        case PCR_HIP_CRS_GEOGRAPHIC: {
            if (!(fabs(y) <= 90.0) || !(fabs(x) < INFINITY)) return false;
            g->lon = x;
            g->phi = y * kD2R;
            sincos(g->phi, &g->s, &g->c);
            return true;
        }
        case PCR_HIP_CRS_WEB_MERCATOR: {
            // psi = y / a is the isometric latitude of the sphere: sin phi = tanh psi, cos phi = 1 / cosh psi
            // with E = exp(-|psi|): tanh|psi| = (1 - E^2) / (1 + E^2), 1 / cosh psi = 2 E / (1 + E^2); 1 - E^2 from expm1, so
            // that neither cancels (near the equator 1 - E^2, near the poles anything derived from 1 - E)
            const double psi = y / d.a;
            if (!(fabs(x) < INFINITY) || !(fabs(psi) < INFINITY)) return false;
            const double em = expm1(-fabs(psi)), E = exp(-fabs(psi));
            const double iq = 1.0 / (1.0 + E * E);
            g->s = copysign(-em * (2.0 + em) * iq, psi);
            g->c = 2.0 * E * iq;
            g->lon = x / d.a * kR2D;
            if (need_phi) g->phi = atan2(g->s, g->c);
            return true;
        }
        default: {                                                          // Transverse Mercator, inverse
            const double ika = 1.0 / d.ka, xi = (y - d.fn) * ika, eta = (x - d.fe) * ika;
            // far outside, the beta series is garbage that can fall back inside the cut; up to here eta' rises with eta
            // (NaN and infinite eastings fail too).  The domain tests only gather in `ok`: one branch, at the end
            bool ok = fabs(eta) <= 2.0 * kTmEtaMax;
            double s2x, c2x;
            sincos(2.0 * xi, &s2x, &c2x);
            const double e2 = exp(2.0 * eta);
            const double sh2y = 0.5 * (e2 - 1.0 / e2), ch2y = 0.5 * (e2 + 1.0 / e2);
            double dr, di;
            clenshaw_sin(d.beta, s2x, c2x, sh2y, ch2y, &dr, &di);
            const double xip = xi - dr, etap = eta - di;                    // zeta' = zeta - sum beta_j sin(2 j zeta)
            // what the forward direction refuses, and northings beyond the pole (a few ulp of slack: the pole row itself,
            // rounded up, is the pole); NaN and infinite northings fail here
            ok = ok && fabs(etap) <= kTmEtaMax && fabs(xip) <= 0.5 * kPi * (1.0 + 1e-15);
            double sxp, cxp;
            sincos(xip, &sxp, &cxp);
            cxp = fabs(cxp);                                                // (below zero only within that slack)
            double shp, chp;
            sinh_cosh(etap, &shp, &chp);
            // conformal latitude chi: sin chi = sin xi' / cosh eta', cos chi = sqrt(sinh^2 eta' + cos^2 xi') / cosh eta'
            const double r = sqrt(shp * shp + cxp * cxp);
            const double ich = 1.0 / chp, sch = sxp * ich, cch = r * ich;
            const double chi = atan2(sxp, r);
            const double s2c = 2.0 * sch * cch, c2c = (cch - sch) * (cch + sch);
            // phi = chi + sum delta_j sin(2 j chi): the same Clenshaw with a real argument
            const double a2 = 2.0 * c2c;
            double b1 = 0.0, b2 = 0.0;
            for (int k = 5; k >= 0; --k) {
                const double t = d.delta[k] + a2 * b1 - b2;
                b2 = b1;
                b1 = t;
            }
            g->phi = chi + s2c * b1;
            const double dl = atan2(shp, cxp) * kR2D;
            g->lon = norm_deg(d.lon0 + dl);
            if (!(ok && fabs(dl) < 90.0 && fabs(g->phi) <= 0.5 * kPi)) return false;
            sincos(g->phi, &g->s, &g->c);
            return true;
        }
    }
}

// ---- geographic -> destination -------------------------------------------------------------------------------------------
PCR_HD inline bool encode(const pcr_hip_crs_desc& d, int kind, const Geo& g, double* x, double* y) {
    switch (kind) {
        case PCR_HIP_CRS_GEOGRAPHIC:
            *x = g.lon;
            *y = g.phi * kR2D;
            return true;
        case PCR_HIP_CRS_WEB_MERCATOR: {
            if (!(fabs(g.s) < 1.0) || !(g.c > 0.0)) return false;           // the poles map to infinity
            *x = d.a * (norm_deg(g.lon) * kD2R);
            *y = d.a * asinh(g.s / g.c);                                   // = atanh(sin phi), without its 1 / cos^2 phi
                                                                            // amplification of an error in sin phi
            return true;
        }
        default: {                                                          // Transverse Mercator, forward
            const double dl = norm_deg(g.lon - d.lon0);
            // 90 degrees and more from the central meridian (the poles: at any longitude)
            if (!(fabs(dl) < 90.0) && !(fabs(g.s) == 1.0 && dl == dl)) return false;
            double sl, cl;
            sincos(dl * kD2R, &sl, &cl);
            // tau' = tan(conformal latitude) = tau cosh(sigma) - sinh(sigma) sqrt(1 + tau^2), sigma = e atanh(e sin phi);
            // every quantity below is scaled by cos phi, which cancels: no tan phi, no division by cos phi
            double sh, ch;
            sinh_cosh_sigma(d.e, g.s, &sh, &ch);
            const double T = g.s * ch - sh;                                 // tau' cos phi (sqrt(1 + tau^2) cos phi = 1)
            const double C = g.c * cl, S = g.c * sl;
            const double ir = 1.0 / sqrt(T * T + C * C);
            const double sxp = T * ir, cxp = C * ir, z = S * ir;
            const double xip = atan2(T, C);
            // eta' = asinh(z) = log1p(|z| + z^2 / (1 + sqrt(1 + z^2))) with sign; w = exp(|eta'|)
            const double az = fabs(z);
            const double u = az + az * az / (1.0 + sqrt(1.0 + az * az));
            const double etap = copysign(log1p(u), z);
            const double w2 = (1.0 + u) * (1.0 + u);
            const double sh2y = copysign(0.5 * (w2 - 1.0 / w2), z), ch2y = 0.5 * (w2 + 1.0 / w2);
            const double s2x = 2.0 * sxp * cxp, c2x = (cxp - sxp) * (cxp + sxp);
            double dr, di;
            clenshaw_sin(d.alpha, s2x, c2x, sh2y, ch2y, &dr, &di);
            *x = d.fe + d.ka * (etap + di);
            *y = d.fn + d.ka * (xip + dr);
            return fabs(z) <= kTmSinhEtaMax;                                // the cut on eta' = asinh(z): a compare on what
                                                                            // is already there, no branch ahead of the series
        }
    }
}

// One point.  Descriptors of the same code never get here (the callers copy).  Two geographic CRSs share the datum: the
// coordinates pass unchanged.
PCR_HD inline void transform_point(const pcr_hip_crs_desc& src, const pcr_hip_crs_desc& dst, int sk, int dk, double x, double y,
                                   double* ox, double* oy) {
    double u = NAN, v = NAN;
    if (sk == PCR_HIP_CRS_GEOGRAPHIC && dk == PCR_HIP_CRS_GEOGRAPHIC) {
        if (fabs(y) <= 90.0 && fabs(x) < INFINITY) { u = x; v = y; }
    } else {
        Geo g;
        if (!decode(src, sk, x, y, dk == PCR_HIP_CRS_GEOGRAPHIC, &g) || !encode(dst, dk, g, &u, &v)) u = v = NAN;
    }
    if (u == u && v == v) {
        *ox = u;
        *oy = v;
        return;
    }
    *ox = NAN;                              // a coordinate that is NaN on either axis takes the other with it
    *oy = NAN;
}

}  // namespace crs
}  // namespace pcrhip
