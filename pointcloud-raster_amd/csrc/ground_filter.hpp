// ground_filter.hpp -- the contract of ground_filter (a progressive morphological filter on one band) and of band_difference,
// for the device (csrc/ground_filter.hip) and the host (host/src/ground_filter.h): both compile these lines.
//
// ground_filter(src, radii[1..K], thresholds[1..K]) -> dst, out of place, one Float32 band of height x width cells, NaN = no data.
//   erode(A, R)(r, c)   the minimum of the non-NaN cells of A in rows r-R..r+R and columns c-R..c+R clipped to the image, NaN when
//                       there is none; dilate: the same with the maximum.  Windows are squares: both operators are separable.
//                       NaN cells are ignored, never propagated (minNum / maxNum: fminf / fmaxf, v_min_f32 / v_max_f32).
//   A0 = src.  For k = 1..K:  Ok = dilate(erode(Ak-1, Rk), Rk).  A cell with non-NaN src becomes NON-GROUND when
//                       Ak-1(c) - Ok(c) > tk: one binary32 subtraction rounded to nearest, a NaN difference compares false.
//                       Then Ak = Ok.  Once non-ground, a cell stays non-ground.
//   dst(c) = src(c) bit for bit where src(c) is not NaN and the cell never became non-ground; 0x7FC00000 everywhere else.
//   +-Inf and denormals are values.  1 <= K <= 64, 1 <= R1 < R2 < ... <= 64, every tk finite and >= 0.
// Minimum and maximum are exact and the opened surfaces never leave the function (so the sign of a zero cannot reach dst):
// dst does not depend on the evaluation order or on how a window is decomposed, and device and host agree bit for bit.
//
// band_difference: hag(c) = top(c) - ground(c), one binary32 subtraction; 0x7FC00000 when an operand or the result is NaN.
//
// line_window is how both sides evaluate a one-dimensional window.  Up to R = 4 a window's 2R + 1 cells are walked; beyond,
// the cost does not grow with R (van Herk / Gil-Werman): the line is cut into segments of n = 2R + 1 cells, the suffix minima
// of a segment and the prefix minima of the next one meet in every window, three operations per cell.  It works in place on
// a line the caller staged with an apron of R cells either side (cells outside the image as NaN).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PCR_GF_HD __host__ __device__ __forceinline__
#else
#define PCR_GF_HD inline
#endif
#if defined(__clang__)
#define PCR_GF_UNROLL _Pragma("unroll")
#else
#define PCR_GF_UNROLL _Pragma("GCC unroll 16")
#endif

namespace pcrhip {
namespace ground {

constexpr int kMaxRadius = 64;
constexpr int kMaxLevels = 64;

PCR_GF_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

// a cell as it enters the filter: every NaN is the one quiet NaN, so that fminf / fmaxf never meet a signalling one (libraries
// and machines disagree on those); everything else bit for bit
PCR_GF_HD float clean(float x) { return x != x ? nodata() : x; }

template <bool MAX>
PCR_GF_HD float pick(float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); }

// L[i * step], i = 0 .. T + 2R - 1, holds a line whose cell i is the image cell at position i - R of the T cells wanted.  On
// return L[o * step], o = 0 .. T - 1, is the minimum (MAX: maximum) of the non-NaN cells among the line's cells o .. o + 2R,
// i.e. of the window of radius R around wanted cell o; the cells from T on are scratch.
// Both forms below work through the line in groups of kGroup cells: all loads of a group, then its arithmetic, then its
// stores.  A group's stores never touch what a later group loads, so nothing is lost; what is gained is that a lane that
// evaluates a line in LDS waits for one round trip per group, not one per cell.
constexpr int kGroup = 8;

// R <= 4: window o is walked directly, 2R + 1 cells per output (fewer operations than segments of 3 .. 9 cells would take).
// Output o overwrites cell o, which no later window reads.
template <bool MAX, int R>
PCR_GF_HD void line_window_walk(float* L, int step, int T) {
    for (int o = 0; o < T; o += kGroup) {
        float x[kGroup + 2 * R];
PCR_GF_UNROLL
        for (int i = 0; i < kGroup + 2 * R; ++i) x[i] = o + i < T + 2 * R ? L[(o + i) * step] : nodata();
PCR_GF_UNROLL
        for (int k = 0; k < kGroup; ++k) {
            float m = x[k];
PCR_GF_UNROLL
            for (int d = 1; d <= 2 * R; ++d) m = pick<MAX>(m, x[k + d]);
            if (o + k < T) L[(o + k) * step] = m;
        }
    }
}

template <bool MAX>
PCR_GF_HD void line_window(float* L, int step, int R, int T) {
    switch (R) {
        case 1: return line_window_walk<MAX, 1>(L, step, T);
        case 2: return line_window_walk<MAX, 2>(L, step, T);
        case 3: return line_window_walk<MAX, 3>(L, step, T);
        case 4: return line_window_walk<MAX, 4>(L, step, T);
        default: break;
    }
    const int n = 2 * R + 1;
    for (int s = 0; s < T; s += n) {
        // suffix minima of segment s .. s + n - 1 (always inside the line: s + n - 1 <= T - 1 + 2R), in place
        float acc = nodata();
        for (int p = s + n - 1; p >= s; p -= kGroup) {
            float x[kGroup];
PCR_GF_UNROLL
            for (int k = 0; k < kGroup; ++k) x[k] = p - k >= s ? L[(p - k) * step] : nodata();
PCR_GF_UNROLL
            for (int k = 0; k < kGroup; ++k) {
                acc = pick<MAX>(x[k], acc);
                x[k] = acc;
            }
PCR_GF_UNROLL
            for (int k = 0; k < kGroup; ++k)
                if (p - k >= s) L[(p - k) * step] = x[k];
        }
        // window o = s + j ends j - 1 cells into the next segment, which still holds the line's cells
        const int m = T - s < n ? T - s : n;
        float g = nodata();
        for (int j = 1; j < m; j += kGroup) {
            float a[kGroup], h[kGroup];
PCR_GF_UNROLL
            for (int k = 0; k < kGroup; ++k) {
                a[k] = j + k < m ? L[(s + n + j + k - 1) * step] : nodata();
                h[k] = j + k < m ? L[(s + j + k) * step] : nodata();
            }
PCR_GF_UNROLL
            for (int k = 0; k < kGroup; ++k) {
                g = pick<MAX>(g, a[k]);
                h[k] = pick<MAX>(h[k], g);
            }
PCR_GF_UNROLL
            for (int k = 0; k < kGroup; ++k)
                if (j + k < m) L[(s + j + k) * step] = h[k];
        }
    }
}

// the verdict of one level on one cell: a = A(k-1)(c), o = Ok(c)
PCR_GF_HD bool non_ground(float a, float o, float t) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, o) > t;
#else
    const volatile float d = a - o;                             // one binary32 subtraction, whatever the host evaluates floats in
    return d > t;
#endif
}

PCR_GF_HD float difference(float top, float gnd) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float d = __fsub_rn(top, gnd);
#else
    const volatile float dv = top - gnd;
    const float d = dv;
#endif
    return d != d ? nodata() : d;
}

}  // namespace ground
}  // namespace pcrhip
