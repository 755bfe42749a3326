// extremes.hpp -- the arithmetic of the per-cell extremes (pcr_hip_scatter_extremes, pcr_hip_extremes_band,
// PipelineConfig::extremes), for the device (csrc/extremes.hip), the C-ABI's host twin and the host engine
// (host/src/extremes.cpp, host_engine.cpp): all compile these lines, with contraction off, so key planes kept in HBM and planes
// kept by the host loop, and the bands walked out of either, agree bit for bit.  The contract is written in include/pcr_hip.h
// ("per-cell extremes") and DESIGN.md section 21.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PCR_EXT_HD __host__ __device__ __forceinline__
#else
#define PCR_EXT_HD inline
#endif

namespace pcrhip {
namespace ext {

constexpr int kMinK = 2, kMaxK = 8;             // PCR_HIP_EXTREMES_MIN_K, PCR_HIP_EXTREMES_MAX_K
constexpr int kLowest = 0, kHighest = 1;        // PCR_HIP_EXTREMES_LOWEST, PCR_HIP_EXTREMES_HIGHEST
constexpr uint32_t kEmpty = 0xFFFFFFFFu;        // an empty slot, and the word of a NaN value: above every real value's key

// ord() maps float bits monotonically onto unsigned integers (select_ord of common.hpp, the MostRecent fold's): -Inf ->
// 0x007FFFFF, +-0 -> 0x80000000, +Inf -> 0xFF800000.
PCR_EXT_HD uint32_t ord(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
PCR_EXT_HD uint32_t unord(uint32_t u) { return (u >> 31) ? (u ^ 0x80000000u) : ~u; }

// The key of a value: its bits, -0.0 folded to +0.0 on the bits, ord() for Lowest, ~ord() for Highest -- the smaller the key
// the more extreme the value.  Every real value's key lies in [0x007FFFFF, 0xFF800000] on either side; a NaN gives kEmpty.
PCR_EXT_HD uint32_t key_of(float v, int side) {
    if (v != v) return kEmpty;
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    if (b == 0x80000000u) b = 0u;
    const uint32_t o = ord(b);
    return side == kHighest ? ~o : o;
}
PCR_EXT_HD float value_of(uint32_t key, int side) {
    const uint32_t b = unord(side == kHighest ? ~key : key);
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}

PCR_EXT_HD float nodata() {
    const uint32_t bits = 0x7FC00000u;
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

// Sorted insertion of one key into a cell's k slots, `stride` words apart, ascending, distinct, kEmpty behind the filled ones:
// what a single owner of the cell does (the host engine; the device merges lists the same way).  A key at or above the last
// slot, or one that is there already, changes nothing.
PCR_EXT_HD void insert_sorted(uint32_t* slot, int64_t stride, int k, uint32_t key) {
    if (key >= slot[(int64_t)(k - 1) * stride]) return;
    int j = 0;
    while (slot[(int64_t)j * stride] < key) ++j;                       // (ends: the last slot is above the key)
    if (slot[(int64_t)j * stride] == key) return;
    for (int m = k - 1; m > j; --m) slot[(int64_t)m * stride] = slot[(int64_t)(m - 1) * stride];
    slot[(int64_t)j * stride] = key;
}

// The band of one cell from its k keys (ascending, kEmpty behind the n filled ones): NaN where n == 0; else start at i = 0 and
// advance while i + 1 < n and d > max_gap, d being ONE binary32 subtraction, v[i+1] - v[i] for Lowest and v[i] - v[i+1] for
// Highest (distinct keys: never NaN, +Inf between -Inf and anything else); the band is v[i].  max_gap = +Inf: the plain Min /
// Max.  A cell whose kept values are all more than max_gap apart yields the last of them, the k-th when all slots are filled.
// values: null, or where the k decoded values go, `vstride` floats apart (NaN for an empty slot).
PCR_EXT_HD float band_of(const uint32_t* keys, int64_t stride, int k, int side, float max_gap, float* values, int64_t vstride) {
    // (every index below is a constant once the loops are unrolled: the values stay in registers on the device)
    float v[kMaxK];
    int n = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < kMaxK; ++j) {
        v[j] = nodata();
        if (j >= k) continue;
        const uint32_t key = keys[(int64_t)j * stride];
        if (key != kEmpty) {
            v[j] = value_of(key, side);
            n = j + 1;
        }
        if (values) values[(int64_t)j * vstride] = v[j];
    }
    float cur = v[0];                                                  // (NaN where n == 0)
    bool walking = true;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 1; j < kMaxK; ++j) {
        if (!walking || j >= n) continue;
        const float d = side == kHighest ? cur - v[j] : v[j] - cur;
        if (d > max_gap) cur = v[j];
        else walking = false;
    }
    return cur;
}

}  // namespace ext
}  // namespace pcrhip
