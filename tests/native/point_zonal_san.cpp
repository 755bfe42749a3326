// point_zonal_san.cpp -- the host twins' loops of the point zonal tables (csrc/point_zonal.hpp) under AddressSanitizer + UBSan,
// on the CPU: every edge label (Z, Z + 1, 2^24, 2^24 + 2, 0, -0.0, -1, 2.5, NaN, +-Inf) with mask bytes 0, 1, 255 and none,
// values NaN, +-Inf, at the +-2^21 step clamp and one step inside it, 1, 63, 64, 65 and 256 bins, tables seeded with 2^64 - 3 so
// that every sum wraps, info words, n = 0.  Labels, masks, values and tables are allocated exactly (no slack: ASan sees the first
// element outside any of them), and every table is compared with sums made here another way: per zone, over the points of that
// zone, in unsigned __int128.  Built and run by tests/test_point_zonal.py.
#include "point_zonal.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>

namespace {

namespace pz = pcrhip::pzonal;
namespace cs = pcrhip::cs;
namespace hist = pcrhip::hist;
using u64 = unsigned long long;
using u128 = unsigned __int128;

void fail(const char* what) {
    std::printf("FAILED: %s\n", what);
    std::exit(1);
}

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {            // a copy with no slack behind it
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

constexpr u64 kSeed = ~0ull - 2;                                 // 2^64 - 3

void run(uint32_t Z, int bins, bool masked, uint64_t n_points, u64 seed) {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const double origin = 1.5, inv_res = 8.0, res = 0.125, lo = -3.0, inv_w = bins / 64.0;
    const float edge_labels[] = {(float)Z, (float)Z + 1.0f, 16777216.0f, 16777218.0f, 0.0f, -0.0f, -1.0f, 2.5f, nan, inf, -inf, 1.0f, 2.0f, 1.0f};
    const float edge_values[] = {nan, inf, -inf, (float)(origin + cs::kQ * res), (float)(origin - cs::kQ * res),
                                 (float)(origin + (cs::kQ - 1) * res), (float)(origin - (cs::kQ - 1) * res), -7.25f, 0.0f, 63.9f, -3.0f, 61.0f};
    const uint8_t mask_bytes[] = {0, 1, 255, 1, 1};
    std::vector<float> label, value;
    std::vector<uint8_t> mask;
    for (uint64_t i = 0; i < n_points; ++i) {                    // every label meets every value and every mask byte
        label.push_back(i % 3 == 0 ? edge_labels[(i / 3) % 14] : (float)(1 + (i / 7) % Z));
        value.push_back(edge_values[i % 12]);
        mask.push_back(mask_bytes[(i / 5) % 5]);
    }
    auto L = exact(label), V = exact(value);
    auto M = exact(mask);
    const uint8_t* m = masked ? M.get() : nullptr;
    std::vector<u64> points(Z, seed), zn(Z, seed), zs2(Z, seed), counts((size_t)Z * bins, seed), info{3, seed}, info_h{0, 0};
    std::vector<long long> zs1(Z, (long long)seed);
    auto P = exact(points), N = exact(zn), S2 = exact(zs2), C = exact(counts), I = exact(info), IH = exact(info_h);
    auto S1 = exact(zs1);
    pz::fold_stats_host(L.get(), m, V.get(), n_points, origin, inv_res, Z, P.get(), N.get(), S1.get(), S2.get(), I.get());
    pz::fold_hist_host(L.get(), m, V.get(), n_points, bins, lo, inv_w, Z, C.get(), IH.get());

    // the same sums zone by zone
    u64 zmax = 3, over = seed, zmax_h = 0, over_h = 0;
    for (uint64_t i = 0; i < n_points; ++i) {
        if (m && !m[i]) continue;
        const uint32_t z = pcrhip::zonal::zone_of(L[i]);
        if (z > Z) { over += 1; over_h += 1; }
        else if (z) { zmax = z > zmax ? z : zmax; zmax_h = z > zmax_h ? z : zmax_h; }
    }
    if (I[0] != zmax || I[1] != over || IH[0] != zmax_h || IH[1] != over_h) fail("info words");
    for (uint32_t z = 1; z <= Z; ++z) {
        u128 p = seed, c = seed, a = seed, b = seed;
        std::vector<u128> row((size_t)bins, seed);
        for (uint64_t i = 0; i < n_points; ++i) {
            if ((m && !m[i]) || pcrhip::zonal::zone_of(L[i]) != z) continue;
            p += 1;
            const int32_t q = cs::step_of(V[i], origin, inv_res);
            if (q != cs::kNoStep) {
                c += 1;
                a += (u128)(u64)(long long)q;                    // two's complement, modulo 2^64
                b += (u128)((long long)q * (long long)q);
            }
            const uint32_t bin = hist::bin_of(V[i], lo, inv_w, bins);
            if (bin != hist::kNoBin) row[bin] += 1;
        }
        if (P[z - 1] != (u64)p || N[z - 1] != (u64)c || (u64)S1[z - 1] != (u64)a || S2[z - 1] != (u64)b) fail("stats tables");
        for (int k = 0; k < bins; ++k)
            if (C[(size_t)(z - 1) * bins + k] != (u64)row[(size_t)k]) fail("histogram table");
    }
}

}  // namespace

int main() {
    for (uint32_t Z : {1u, 9u})
        for (int bins : {1, 63, 64, 65, 256})
            for (bool masked : {false, true})
                for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)63, (uint64_t)64, (uint64_t)65, (uint64_t)200, (uint64_t)1260})
                    for (u64 seed : {0ull, kSeed}) run(Z, bins, masked, n, seed);
    {   // points alone; no info words; no points table
        const std::vector<float> label{1.0f, 2.0f, 2.0f, 3.0f, 4.0f};
        auto L = exact(label), V = exact(label);
        std::vector<u64> t(3, 0);
        auto P = exact(t), N = exact(t), S2 = exact(t);
        std::vector<long long> s(3, 0);
        auto S1 = exact(s);
        pz::fold_stats_host(L.get(), nullptr, nullptr, 5, 0.0, 1.0, 3, P.get(), nullptr, nullptr, nullptr, nullptr);
        if (P[0] != 1 || P[1] != 2 || P[2] != 1) fail("points alone");
        pz::fold_stats_host(L.get(), nullptr, V.get(), 5, 0.0, 1.0, 3, nullptr, N.get(), S1.get(), S2.get(), nullptr);
        if (N[1] != 2 || S1[1] != 4 || S2[1] != 8 || S2[2] != 9) fail("no points table");
    }
    std::printf("the twins' loops survived\n");
    return 0;
}
