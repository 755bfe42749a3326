// zone_rows.h -- (internal) what the zonal tables (zonal.h: one row per zone of a label BAND) and the point zonal tables
// (point_zonal.h: of a label CHANNEL) share once their integer tables are folded: the arena their pieces come from, the ONE
// routine that turns the integer tables into a table's columns -- the C-ABI's row kernels on device memory, their host twins on
// host memory -- and the ONE rule that names and orders the columns, which the Python bindings use too.
#pragma once

#include "buffer.h"
#include "pcr/engine/pipeline.h"
#include "pipeline_common.h"

#include <string>
#include <vector>

namespace pcr {
namespace detail {

/// The pieces of one call in one allocation of `loc` memory: handed out on 256 bytes.
struct Arena {
    Buffer buf;
    size_t used = 0;
    static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(static_cast<char*>(buf.data()) + used);
        used += padded(count * sizeof(T));
        return p;
    }
};

/// What a table's columns are made from: per stats spec and per histogram the folded integer tables (in `loc` memory, at least Z
/// rows each) and the constants of its rows.
struct ZoneRowsInputs {
    struct Stat {
        std::string channel;
        const unsigned long long* n = nullptr;
        const long long* s1 = nullptr;
        const unsigned long long* s2 = nullptr;
        double origin = 0.0, resolution = 0.0;
        int ddof = 0;
    };
    struct Hist {
        std::string channel;
        const unsigned long long* counts = nullptr;      // [zone][bin]
        int bins = 0;
        double lo = 0.0, w = 0.0;
        std::vector<float> q;
    };
    const unsigned long long* count = nullptr;   // the count column: `cells` or `points`
    std::vector<Stat> stats;
    std::vector<Hist> hists;
};

/// The columns of a table of Z rows, zones 1 .. Z: the float columns and hist_n are made in an arena of `loc` memory (on `stream`
/// on the device), every column is copied out, and the stream is waited for once.  Z == 0: the columns' channels, bins and
/// percentiles alone.  with_counts: the histograms' [zone][bin] counts are copied out too.  On failure everything is left empty.
Status zone_rows(MemoryLocation loc, void* stream, size_t Z, const ZoneRowsInputs& in, bool with_counts, std::vector<int32_t>& zone,
                 std::vector<int64_t>& count, std::vector<ZonalTable::StatColumns>& stats, std::vector<ZonalTable::HistColumns>& hists);

/// The columns of a table by name, in the order of Pipeline.zonal's and Pipeline.point_zonal's dict: f(name, column) for "zone",
/// the count column (`count_name`: "cells" or "points"), per stats spec "{channel}_n", "_mean", "_var", "_std", per histogram
/// "{channel}_hist_n" and one percentile_name per percentile.
template <class F>
void for_each_zone_column(const std::vector<int32_t>& zone, const char* count_name, const std::vector<int64_t>& count,
                          const std::vector<ZonalTable::StatColumns>& stats, const std::vector<ZonalTable::HistColumns>& hists, F&& f) {
    f(std::string("zone"), zone);
    f(std::string(count_name), count);
    for (const auto& c : stats) {
        f(c.channel + "_n", c.n);
        f(c.channel + "_mean", c.mean);
        f(c.channel + "_var", c.var);
        f(c.channel + "_std", c.stddev);
    }
    for (const auto& c : hists) {
        f(c.channel + "_hist_n", c.hist_n);
        for (size_t j = 0; j < c.q.size(); ++j) f(percentile_name(c.channel, c.q[j]), c.p[j]);
    }
}
/// ... the names alone, of the table these specs would give (their channels and percentiles are all that is read), and create()'s
/// refusal of a table in which one appears twice: "<where>: column '<name>' appears twice".
std::vector<std::string> zone_column_names(const char* count_name, const ZoneRowsInputs& specs);
Status check_zone_column_names(const std::string& where, const char* count_name, const ZoneRowsInputs& specs);

}  // namespace detail
}  // namespace pcr
