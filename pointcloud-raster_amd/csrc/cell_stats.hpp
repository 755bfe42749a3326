// cell_stats.hpp -- the arithmetic of the per-cell spread (pcr_hip_scatter_cell_stats, pcr_hip_cell_stats_bands,
// PipelineConfig::cell_stats), for the device (csrc/cell_stats.hip), the C-ABI's host twin and the host engine
// (host/src/cell_stats.cpp, host_engine.cpp): all compile these lines, with contraction off, so planes summed in HBM and planes
// summed by the host loop, and the bands made from either, agree bit for bit.  The contract is written in include/pcr_hip.h
// ("per-cell stats") and DESIGN.md section 22.
//
// The state is three INTEGER planes -- N, S1 = sum of q, S2 = sum of q^2 over the accepted points of a cell, q the value
// quantized to a step -- so the fold is integer addition (any order, any chunking, the same bits) and the variance numerator
// N * S2 - S1^2 is an exact 128-bit integer: nothing cancels, whatever the offset of the values.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCR_CS_HD __host__ __device__ __forceinline__
#else
#define PCR_CS_HD inline
#endif

namespace pcrhip {
namespace cs {

constexpr int kMean = 0, kVariance = 1, kStdDev = 2;   // PCR_HIP_CELL_STAT_MEAN, _VARIANCE, _STDDEV
constexpr int kMaxProducts = 3;                        // PCR_HIP_CELL_STATS_MAX_PRODUCTS
constexpr int32_t kQ = 1 << 21;                        // PCR_HIP_CELL_STATS_Q: |q| <= kQ
constexpr int32_t kNoStep = INT32_MIN;                 // the word of a NaN value: the point is not counted

// The step of a value, binary64: t = (v - origin) * inv_res, one subtraction and one multiplication (nothing to contract);
// at or beyond -+kQ, -+Inf included: clamped (counted, like the histogram's end bins); else rint(t), ties to even.  NaN: kNoStep.
PCR_CS_HD int32_t step_of(float v, double origin, double inv_res) {
    if (v != v) return kNoStep;
    const double t = ((double)v - origin) * inv_res;
    if (t <= -(double)kQ) return -kQ;
    if (t >= (double)kQ) return kQ;
    return (int32_t)__builtin_rint(t);
}

PCR_CS_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

// a * b as (hi, lo), exact: the one place that differs between the device and the host.  (No __int128 conversion or division
// is relied on in device code.)
PCR_CS_HD void mul64(uint64_t a, uint64_t b, uint64_t& hi, uint64_t& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    hi = __umul64hi(a, b);
    lo = a * b;
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    hi = (uint64_t)(p >> 64);
    lo = (uint64_t)p;
#endif
}

// D = N * S2 - S1^2 as an unsigned 128-bit integer (hi, lo): one 64 x 64 -> 128 multiply for each term, one subtraction with
// borrow.  Non-negative (Cauchy-Schwarz) while no plane has wrapped; modulo 2^128 otherwise.
PCR_CS_HD void numerator(uint32_t n, int64_t s1, uint64_t s2, uint64_t& hi, uint64_t& lo) {
    uint64_t ah, al, bh, bl;
    mul64((uint64_t)n, s2, ah, al);
    const uint64_t a = s1 < 0 ? (uint64_t)0 - (uint64_t)s1 : (uint64_t)s1;
    mul64(a, a, bh, bl);
    lo = al - bl;
    hi = ah - bh - (al < bl ? 1u : 0u);
}

// The mean of a cell with n >= 1: every operation rounded on its own.
PCR_CS_HD float mean_of(uint32_t n, int64_t s1, double origin, double resolution) {
    const double mq = (double)s1 / (double)n;
    const double off = resolution * mq;
    return (float)(origin + off);
}

// The variance of a cell in steps^2, binary64, n > ddof: D / (N * (N - ddof)), D converted as hi * 2^64 + lo.
PCR_CS_HD double variance_steps(uint32_t n, int64_t s1, uint64_t s2, int ddof) {
    uint64_t hi, lo;
    numerator(n, s1, s2, hi, lo);
    const double dh = (double)hi * 0x1p64;
    const double dd = dh + (double)lo;
    const double den = (double)n * (double)(n - (uint32_t)ddof);
    return dd / den;
}

// The bands of one cell.  res2 = resolution * resolution, computed once by the caller.  NaN where n == 0; the spread also
// where n <= ddof.  sqrt and / are the correctly rounded binary64 operations (as in terrain.hpp).
PCR_CS_HD void bands_of(uint32_t n, int64_t s1, uint64_t s2, double origin, double resolution, double res2, int ddof, float& mean,
                        float& variance, float& stddev) {
    mean = variance = stddev = nodata();
    if (n == 0) return;
    mean = mean_of(n, s1, origin, resolution);
    if (n <= (uint32_t)ddof) return;
    const double vq = variance_steps(n, s1, s2, ddof);
    variance = (float)(res2 * vq);
    stddev = (float)(resolution * __builtin_sqrt(vq));
}

}  // namespace cs
}  // namespace pcrhip
