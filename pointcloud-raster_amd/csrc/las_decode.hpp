// las_decode.hpp -- one LAS point record -> x, y (Float64) and the Float32 channels, given a pcr_hip_las_layout
// (include/pcr_hip.h).  __host__ __device__: las_decode.hip compiles it into the gfx950 kernel and into
// pcr_hip_las_decode_host -- one source for both, and the only place that knows where a field sits in a record
// (ASPRS LAS 1.4 R15, tables 7-18: point data record formats 0-10).  Little-endian.
//
// A record is read through a byte reader `rd(offset) -> unsigned` and every wider field is assembled from its bytes: the
// fields are not naturally aligned (an f64 at byte 20 or 22 of a 28-, 34- or 30-byte record), so no pointer to one is
// ever formed.  Coordinates are one multiply and one add, each rounded ((double)X * scale + offset; both builds compile
// with -ffp-contract=off) -- what every LAS reader computes.
#pragma once

#include <cstdint>

#include "pcr_hip.h"

#if defined(__HIPCC__)
#define PCR_HD __host__ __device__
#else
#define PCR_HD
#endif

namespace pcrhip {
namespace las {

constexpr int kMaxFormat = 10;

// Smallest record of a point format; a longer record_length means extra bytes after it.
PCR_HD inline int min_record_length(int fmt) {
    switch (fmt) {
        case 0: return 20; case 1: return 28; case 2: return 26; case 3: return 34; case 4: return 57; case 5: return 63;
        case 6: return 30; case 7: return 36; case 8: return 38; case 9: return 59; case 10: return 67;
        default: return 0;
    }
}

PCR_HD inline bool has_gps_time(int fmt) { return fmt == 1 || (fmt >= 3 && fmt <= 10); }
PCR_HD inline bool has_rgb(int fmt) { return fmt == 2 || fmt == 3 || fmt == 5 || fmt == 7 || fmt == 8 || fmt == 10; }
PCR_HD inline bool has_nir(int fmt) { return fmt == 8 || fmt == 10; }

// Bit c set: the format has channel PCR_HIP_LAS_CH_* c.
PCR_HD inline unsigned channel_mask(int fmt) {
    if (fmt < 0 || fmt > kMaxFormat) return 0u;
    unsigned m = (1u << PCR_HIP_LAS_CH_GPS_TIME) - 1u;           // z .. point_source_id: every format
    if (has_gps_time(fmt)) m |= 1u << PCR_HIP_LAS_CH_GPS_TIME;
    if (has_rgb(fmt)) m |= (1u << PCR_HIP_LAS_CH_RED) | (1u << PCR_HIP_LAS_CH_GREEN) | (1u << PCR_HIP_LAS_CH_BLUE);
    if (has_nir(fmt)) m |= 1u << PCR_HIP_LAS_CH_NIR;
    return m;
}

template <class Rd> PCR_HD inline unsigned rd_u16(const Rd& rd, int o) { return rd(o) | (rd(o + 1) << 8); }
template <class Rd> PCR_HD inline unsigned rd_u32(const Rd& rd, int o) {
    return rd(o) | (rd(o + 1) << 8) | (rd(o + 2) << 16) | (rd(o + 3) << 24);
}
template <class Rd> PCR_HD inline double rd_f64(const Rd& rd, int o) {
    const uint64_t u = (uint64_t)rd_u32(rd, o) | ((uint64_t)rd_u32(rd, o + 4) << 32);
    double d;
    __builtin_memcpy(&d, &u, sizeof d);
    return d;
}

PCR_HD inline double coordinate(unsigned raw, double scale, double offset) {
    const double scaled = (double)(int32_t)raw * scale;          // rounded, then the add (no fma)
    return scaled + offset;
}

// NEW: formats 6-10 (true) or 0-5 (false).  `want`: bit c set = channel c is stored through put(c, value); a clear bit costs
// neither the field's reads nor a store (the mask is uniform: scalar branches on the device).  The caller has checked the
// layout (format, record_length >= min_record_length, want within channel_mask).
template <bool NEW, class Rd, class Put>
PCR_HD inline void decode_record(const pcr_hip_las_layout& lay, unsigned want, const Rd& rd, double* x, double* y, const Put& put) {
    *x = coordinate(rd_u32(rd, 0), lay.scale[0], lay.offset[0]);
    *y = coordinate(rd_u32(rd, 4), lay.scale[1], lay.offset[1]);
    if (want & (1u << PCR_HIP_LAS_CH_Z)) put(PCR_HIP_LAS_CH_Z, (float)coordinate(rd_u32(rd, 8), lay.scale[2], lay.offset[2]));
    if (want & (1u << PCR_HIP_LAS_CH_INTENSITY)) put(PCR_HIP_LAS_CH_INTENSITY, (float)rd_u16(rd, 12));
    if (want & ((1u << PCR_HIP_LAS_CH_RETURN_NUMBER) | (1u << PCR_HIP_LAS_CH_NUMBER_OF_RETURNS))) {
        const unsigned b = rd(14);
        if (want & (1u << PCR_HIP_LAS_CH_RETURN_NUMBER)) put(PCR_HIP_LAS_CH_RETURN_NUMBER, (float)(NEW ? (b & 15u) : (b & 7u)));
        if (want & (1u << PCR_HIP_LAS_CH_NUMBER_OF_RETURNS))
            put(PCR_HIP_LAS_CH_NUMBER_OF_RETURNS, (float)(NEW ? (b >> 4) : ((b >> 3) & 7u)));
    }
    if (want & ((1u << PCR_HIP_LAS_CH_CLASSIFICATION) | (1u << PCR_HIP_LAS_CH_WITHHELD) | (1u << PCR_HIP_LAS_CH_OVERLAP))) {
        const unsigned b = rd(15);                               // formats 0-5: classification + flags; 6-10: flags
        const unsigned cls = NEW ? ((want & (1u << PCR_HIP_LAS_CH_CLASSIFICATION)) ? rd(16) : 0u) : (b & 31u);
        if (want & (1u << PCR_HIP_LAS_CH_CLASSIFICATION)) put(PCR_HIP_LAS_CH_CLASSIFICATION, (float)cls);
        if (want & (1u << PCR_HIP_LAS_CH_WITHHELD)) put(PCR_HIP_LAS_CH_WITHHELD, (float)(NEW ? ((b >> 2) & 1u) : (b >> 7)));
        if (want & (1u << PCR_HIP_LAS_CH_OVERLAP)) put(PCR_HIP_LAS_CH_OVERLAP, (float)(NEW ? ((b >> 3) & 1u) : (cls == 12u ? 1u : 0u)));
    }
    if (want & (1u << PCR_HIP_LAS_CH_SCAN_ANGLE)) {
        if (NEW) {
            const double steps = (double)(int16_t)rd_u16(rd, 18);            // 0.006 degree steps
            put(PCR_HIP_LAS_CH_SCAN_ANGLE, (float)(steps * 0.006));
        } else {
            put(PCR_HIP_LAS_CH_SCAN_ANGLE, (float)(int8_t)rd(16));           // scan angle rank, degrees
        }
    }
    if (want & (1u << PCR_HIP_LAS_CH_USER_DATA)) put(PCR_HIP_LAS_CH_USER_DATA, (float)rd(17));
    if (want & (1u << PCR_HIP_LAS_CH_POINT_SOURCE_ID)) put(PCR_HIP_LAS_CH_POINT_SOURCE_ID, (float)rd_u16(rd, NEW ? 20 : 18));
    if (want & (1u << PCR_HIP_LAS_CH_GPS_TIME)) {
        // around 3e8 s Float32 resolves 32 s: the origin is taken off in Float64, before the narrowing
        const double t = rd_f64(rd, NEW ? 22 : 20);
        put(PCR_HIP_LAS_CH_GPS_TIME, (float)(t - lay.gps_time_origin));
    }
    if (want & ((1u << PCR_HIP_LAS_CH_RED) | (1u << PCR_HIP_LAS_CH_GREEN) | (1u << PCR_HIP_LAS_CH_BLUE))) {
        const int o = NEW ? 30 : (lay.point_format == 2 ? 20 : 28);
        if (want & (1u << PCR_HIP_LAS_CH_RED)) put(PCR_HIP_LAS_CH_RED, (float)rd_u16(rd, o));
        if (want & (1u << PCR_HIP_LAS_CH_GREEN)) put(PCR_HIP_LAS_CH_GREEN, (float)rd_u16(rd, o + 2));
        if (want & (1u << PCR_HIP_LAS_CH_BLUE)) put(PCR_HIP_LAS_CH_BLUE, (float)rd_u16(rd, o + 4));
    }
    if (NEW && (want & (1u << PCR_HIP_LAS_CH_NIR))) put(PCR_HIP_LAS_CH_NIR, (float)rd_u16(rd, 36));
}

}  // namespace las
}  // namespace pcrhip
