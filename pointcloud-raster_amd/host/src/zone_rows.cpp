// zone_rows.cpp -- see zone_rows.h.
#include "zone_rows.h"

#include "pcr_hip.h"

#include <algorithm>

namespace pcr {
namespace detail {

namespace {

// The columns' channels, bins and percentiles, no row yet.
void name_columns(const ZoneRowsInputs& in, std::vector<ZonalTable::StatColumns>& stats, std::vector<ZonalTable::HistColumns>& hists) {
    stats.assign(in.stats.size(), {});
    hists.assign(in.hists.size(), {});
    for (size_t k = 0; k < in.stats.size(); ++k) stats[k].channel = in.stats[k].channel;
    for (size_t k = 0; k < in.hists.size(); ++k) {
        hists[k].channel = in.hists[k].channel;
        hists[k].bins = in.hists[k].bins;
        hists[k].q = in.hists[k].q;
        hists[k].p.resize(in.hists[k].q.size());
    }
}

}  // namespace

Status zone_rows(MemoryLocation loc, void* st, size_t Z, const ZoneRowsInputs& in, bool with_counts, std::vector<int32_t>& zone,
                 std::vector<int64_t>& count, std::vector<ZonalTable::StatColumns>& stats, std::vector<ZonalTable::HistColumns>& hists) {
    using u64 = unsigned long long;
    const bool device = loc == MemoryLocation::Device;
    auto fetch = [&](void* dst, const void* src, size_t bytes) { return copy_bytes(dst, MemoryLocation::Host, src, loc, bytes, st); };
    name_columns(in, stats, hists);
    if (Z == 0) return Status::success();

    // the float columns and hist_n, made where the tables live
    size_t bytes = 0;
    for (size_t k = 0; k < in.stats.size(); ++k) bytes += 3 * Arena::padded(Z * 4);
    for (size_t k = 0; k < in.hists.size(); ++k) bytes += Arena::padded(Z * 8) + in.hists[k].q.size() * Arena::padded(Z * 4);
    Arena a;
    Status s = a.buf.allocate(bytes, loc);
    struct StatCols { float *mean, *var, *sd; };
    struct HistCols { u64* n; std::vector<float*> p; };
    std::vector<StatCols> sc(in.stats.size());
    std::vector<HistCols> hc(in.hists.size());
    const uint32_t rows = (uint32_t)Z;
    for (size_t k = 0; k < in.stats.size() && s.ok(); ++k) {
        const ZoneRowsInputs::Stat& p = in.stats[k];
        sc[k] = {a.take<float>(Z), a.take<float>(Z), a.take<float>(Z)};
        s = hip_status(device ? pcr_hip_zone_rows_stats(p.n, p.s1, p.s2, rows, p.origin, p.resolution, p.ddof, sc[k].mean, sc[k].var, sc[k].sd, st)
                              : pcr_hip_zone_rows_stats_host(p.n, p.s1, p.s2, rows, p.origin, p.resolution, p.ddof, sc[k].mean, sc[k].var,
                                                             sc[k].sd));
    }
    for (size_t k = 0; k < in.hists.size() && s.ok(); ++k) {
        const ZoneRowsInputs::Hist& h = in.hists[k];
        hc[k].n = a.take<u64>(Z);
        for (size_t j = 0; j < h.q.size(); ++j) hc[k].p.push_back(a.take<float>(Z));
        const int nq = (int)h.q.size();
        s = hip_status(device ? pcr_hip_zone_rows_percentiles(h.counts, h.bins, rows, h.lo, h.w, nq, h.q.data(), hc[k].n, hc[k].p.data(), st)
                              : pcr_hip_zone_rows_percentiles_host(h.counts, h.bins, rows, h.lo, h.w, nq, h.q.data(), hc[k].n, hc[k].p.data()));
    }

    // the table leaves
    zone.resize(Z);
    for (size_t k = 0; k < Z; ++k) zone[k] = (int32_t)(k + 1);
    count.resize(Z);
    if (s.ok()) s = fetch(count.data(), in.count, Z * 8);
    for (size_t k = 0; k < in.stats.size() && s.ok(); ++k) {
        ZonalTable::StatColumns& c = stats[k];
        c.n.resize(Z);
        c.mean.resize(Z);
        c.var.resize(Z);
        c.stddev.resize(Z);
        s = fetch(c.n.data(), in.stats[k].n, Z * 8);
        if (s.ok()) s = fetch(c.mean.data(), sc[k].mean, Z * 4);
        if (s.ok()) s = fetch(c.var.data(), sc[k].var, Z * 4);
        if (s.ok()) s = fetch(c.stddev.data(), sc[k].sd, Z * 4);
    }
    for (size_t k = 0; k < in.hists.size() && s.ok(); ++k) {
        ZonalTable::HistColumns& c = hists[k];
        c.hist_n.resize(Z);
        s = fetch(c.hist_n.data(), hc[k].n, Z * 8);
        if (with_counts) {
            c.counts.resize(Z * (size_t)c.bins);
            if (s.ok()) s = fetch(c.counts.data(), in.hists[k].counts, c.counts.size() * 8);
        }
        for (size_t j = 0; j < c.p.size() && s.ok(); ++j) {
            c.p[j].resize(Z);
            s = fetch(c.p[j].data(), hc[k].p[j], Z * 4);
        }
    }
    if (device) {
        const Status ws = hip_status(pcr_hip_stream_synchronize(st));         // (the arena is released behind the copies)
        if (s.ok()) s = ws;
    }
    if (!s.ok()) {
        zone.clear();
        count.clear();
        stats.clear();
        hists.clear();
    }
    return s;
}

std::vector<std::string> zone_column_names(const char* count_name, const ZoneRowsInputs& specs) {
    std::vector<ZonalTable::StatColumns> stats;
    std::vector<ZonalTable::HistColumns> hists;
    name_columns(specs, stats, hists);
    std::vector<std::string> names;
    for_each_zone_column({}, count_name, {}, stats, hists,[&](const std::string& name, const auto&) { names.push_back(name); });
    return names;
}

Status check_zone_column_names(const std::string& where, const char* count_name, const ZoneRowsInputs& specs) {
    std::vector<std::string> cols = zone_column_names(count_name, specs);
    std::sort(cols.begin(), cols.end());
    const auto dup = std::adjacent_find(cols.begin(), cols.end());
    return dup == cols.end() ? Status::success() : refuse(where + ": column '" + *dup + "' appears twice");
}

}  // namespace detail
}  // namespace pcr
