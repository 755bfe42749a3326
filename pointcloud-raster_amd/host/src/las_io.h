// las_io.h -- (internal) the file side of LAS input: the public header block and the variable length records in front of
// the point data (ASPRS LAS 1.0-1.4, little-endian), as point_cloud_io.cpp and Pipeline::ingest_file need them.  The records
// themselves are decoded by pcr_hip_las_decode[_host] (csrc/las_decode.hpp); nothing here knows where a field sits in one.
//
// Header-only, so that every program that compiles point_cloud_io.cpp gets it without a further source file.  The parser
// never trusts a length it has not checked against the file size, reads with pread at checked offsets, and allocates at most
// one CRS record (<= 65535 bytes).
#pragma once

#include "../../csrc/las_decode.hpp"
#include "pcr/core/types.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace pcr {
namespace las {

// PCR_HIP_LAS_CH_* -> the channel's name in a cloud (laspy's names)
constexpr const char* kChannelNames[PCR_HIP_LAS_CH_COUNT] = {
    "z", "intensity", "return_number", "number_of_returns", "classification", "withheld", "overlap", "scan_angle",
    "user_data", "point_source_id", "gps_time", "red", "green", "blue", "nir"};

inline int channel_id(const std::string& name) {
    for (int c = 0; c < PCR_HIP_LAS_CH_COUNT; ++c)
        if (name == kChannelNames[c]) return c;
    return -1;
}

struct Header {
    int version_minor = 0;
    uint32_t header_size = 0;
    uint64_t data_offset = 0;
    int point_format = 0;
    uint32_t record_length = 0;
    uint64_t num_points = 0;
    double scale[3] = {1, 1, 1}, offset[3] = {0, 0, 0};
    BBox bounds;
    CRS crs;
    uint64_t file_size = 0;

    unsigned channel_mask() const { return pcrhip::las::channel_mask(point_format); }
    pcr_hip_las_layout layout(double gps_time_origin) const {
        pcr_hip_las_layout l{};
        l.point_format = point_format;
        l.record_length = (int32_t)record_length;
        for (int k = 0; k < 3; ++k) { l.scale[k] = scale[k]; l.offset[k] = offset[k]; }
        l.gps_time_origin = gps_time_origin;
        return l;
    }
};

constexpr const char* kLazMessage = "LAS/LAZ format support not yet implemented (LAZ: compressed point records)";

namespace detail {

inline uint16_t u16_at(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t u32_at(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t u64_at(const uint8_t* p) { return (uint64_t)u32_at(p) | ((uint64_t)u32_at(p + 4) << 32); }
inline double f64_at(const uint8_t* p) {
    const uint64_t u = u64_at(p);
    double d;
    std::memcpy(&d, &u, sizeof d);
    return d;
}

inline bool pread_exact(int fd, void* dst, size_t bytes, uint64_t offset) {
    size_t done = 0;
    while (done < bytes) {
        const ssize_t r = ::pread(fd, static_cast<char*>(dst) + done, bytes - done, (off_t)(offset + done));
        if (r <= 0) return false;
        done += (size_t)r;
    }
    return true;
}

}  // namespace detail

/// `bytes` at `offset` of the file -> dst.  Large reads are cut into 8 MiB pieces handled by a few threads: one thread
/// copying out of the page cache is several times slower than the host-to-device link that takes the records next.
inline bool read_bytes(int fd, void* dst, size_t bytes, uint64_t offset) {
    constexpr size_t kPiece = 8u << 20;
    const size_t pieces = (bytes + kPiece - 1) / kPiece;
    if (pieces <= 1) return detail::pread_exact(fd, dst, bytes, offset);
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    auto work = [&]() {
        for (size_t i = next++; i < pieces; i = next++) {
            const size_t o = i * kPiece;
            if (!detail::pread_exact(fd, static_cast<char*>(dst) + o, std::min(kPiece, bytes - o), offset + o)) ok = false;
        }
    };
    const size_t nthreads = std::min<size_t>({pieces, 8, std::max(1u, std::thread::hardware_concurrency())});
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return ok;
}

namespace detail {

// The CRS of the file from its VLRs in [header_size, data_offset): the OGC WKT record (2112) if there is one, else the
// GeoKeyDirectory (34735).  A VLR that does not fit in front of the point data is an error; a CRS record that cannot be
// used is not (the CRS stays invalid).
inline Status read_vlr_crs(int fd, uint32_t num_vlrs, Header& h) {
    constexpr uint64_t kVlrHeader = 54;
    uint64_t pos = h.header_size;
    std::string wkt;
    int epsg = 0;
    for (uint32_t i = 0; i < num_vlrs; ++i) {
        uint8_t vh[kVlrHeader];
        if (pos + kVlrHeader > h.data_offset || !pread_exact(fd, vh, kVlrHeader, pos))
            return Status::error(StatusCode::IoError, "LAS: variable length record " + std::to_string(i) + " runs past the offset to point data");
        const uint32_t record_id = u16_at(vh + 18), len = u16_at(vh + 20);
        const uint64_t body = pos + kVlrHeader;
        if (body + len > h.data_offset)
            return Status::error(StatusCode::IoError, "LAS: variable length record " + std::to_string(i) + " runs past the offset to point data");
        const bool projection = std::memcmp(vh + 2, "LASF_Projection", 15) == 0;
        if (projection && (record_id == 2112 || record_id == 34735) && len > 0) {
            std::vector<uint8_t> data(len);
            if (!pread_exact(fd, data.data(), len, body)) return Status::error(StatusCode::IoError, "LAS: failed to read a projection record");
            if (record_id == 2112) {
                wkt.assign(reinterpret_cast<const char*>(data.data()), len);
                wkt.resize(std::strlen(wkt.c_str()));                      // NUL padded
            } else if (len >= 8) {
                // GeoKeyDirectory: u16 {version, revision, minor, number of keys}, then {key id, location, count, value} each
                const uint32_t keys = u16_at(data.data() + 6);
                int projected = 0, geographic = 0;
                for (uint32_t k = 0; k < keys && 8 + (uint64_t)(k + 1) * 8 <= len; ++k) {
                    const uint8_t* e = data.data() + 8 + (size_t)k * 8;
                    if (u16_at(e + 2) != 0) continue;                       // the value lives in another record
                    if (u16_at(e) == 3072) projected = u16_at(e + 6);
                    else if (u16_at(e) == 2048) geographic = u16_at(e + 6);
                }
                const int code = projected ? projected : geographic;
                if (code > 0 && code < 32767) epsg = code;                  // 32767: user-defined
            }
        }
        pos = body + len;
    }
    if (!wkt.empty()) h.crs = CRS::from_wkt(wkt);
    else if (epsg) h.crs = CRS::from_epsg(epsg);
    return Status::success();
}

}  // namespace detail

/// The header of an open LAS file.  IoError for anything that is not a readable LAS 1.0-1.4 file whose point records are
/// all there; NotImplemented for LAZ (the compression bits of the point-format byte).
inline Status read_header(int fd, const std::string& path, Header* out) {
    using namespace detail;
    Header h;
    struct stat st;
    if (fd < 0 || ::fstat(fd, &st) != 0 || st.st_size < 0)
        return Status::error(StatusCode::IoError, "failed to open LAS file: " + path + " (note: LAZ support not yet implemented)");
    h.file_size = (uint64_t)st.st_size;
    constexpr size_t kMinHeader = 227, kHeader14 = 375;
    uint8_t b[kHeader14] = {0};
    const size_t have = (size_t)std::min<uint64_t>(h.file_size, kHeader14);
    if (have < kMinHeader || !pread_exact(fd, b, have, 0))
        return Status::error(StatusCode::IoError, "LAS: file is shorter than a LAS header: " + path);
    if (std::memcmp(b, "LASF", 4) != 0) return Status::error(StatusCode::IoError, "LAS: invalid signature (not a LAS file): " + path);
    if (b[24] != 1 || b[25] > 4)
        return Status::error(StatusCode::IoError, "LAS: unsupported version " + std::to_string(b[24]) + "." + std::to_string(b[25]));
    h.version_minor = b[25];
    h.header_size = u16_at(b + 94);
    h.data_offset = u32_at(b + 96);
    const uint32_t num_vlrs = u32_at(b + 100);
    if (h.header_size < kMinHeader || h.header_size > h.file_size)
        return Status::error(StatusCode::IoError, "LAS: header size " + std::to_string(h.header_size) + " does not fit the file");
    if (h.data_offset < h.header_size || h.data_offset > h.file_size)
        return Status::error(StatusCode::IoError, "LAS: offset to point data " + std::to_string(h.data_offset) + " is outside the file");
    if (b[104] & 0xC0) return Status::error(StatusCode::NotImplemented, kLazMessage);
    h.point_format = b[104];
    if (h.point_format > pcrhip::las::kMaxFormat)
        return Status::error(StatusCode::IoError, "LAS: unsupported point format " + std::to_string(h.point_format) + " (0-10)");
    h.record_length = u16_at(b + 105);
    if ((int)h.record_length < pcrhip::las::min_record_length(h.point_format))
        return Status::error(StatusCode::IoError, "LAS: record length " + std::to_string(h.record_length) + " is below the " +
                             std::to_string(pcrhip::las::min_record_length(h.point_format)) + " bytes of point format " +
                             std::to_string(h.point_format));
    h.num_points = u32_at(b + 107);
    if (h.num_points == 0 && h.header_size >= kHeader14 && have >= kHeader14) h.num_points = u64_at(b + 247);
    if (h.num_points > (h.file_size - h.data_offset) / h.record_length)
        return Status::error(StatusCode::IoError, "LAS: truncated file: the header declares " + std::to_string(h.num_points) +
                             " points of " + std::to_string(h.record_length) + " bytes, the file holds fewer");
    for (int k = 0; k < 3; ++k) {
        h.scale[k] = f64_at(b + 131 + 8 * k);
        h.offset[k] = f64_at(b + 155 + 8 * k);
    }
    h.bounds.max_x = f64_at(b + 179);
    h.bounds.min_x = f64_at(b + 187);
    h.bounds.max_y = f64_at(b + 195);
    h.bounds.min_y = f64_at(b + 203);
    Status s = read_vlr_crs(fd, num_vlrs, h);
    if (!s.ok()) return s;
    *out = h;
    return Status::success();
}

/// The wanted channels as a PCR_HIP_LAS_CH_* mask: every channel of the format for an empty list; InvalidArgument for a
/// name that is no LAS channel or one the file's point format lacks.
inline Status wanted_mask(const Header& h, const std::vector<std::string>& names, unsigned* mask) {
    if (names.empty()) { *mask = h.channel_mask(); return Status::success(); }
    *mask = 0u;
    for (const auto& name : names) {
        const int c = channel_id(name);
        if (c < 0)
            return Status::error(StatusCode::InvalidArgument, "LAS: '" + name + "' is not a channel of a LAS file (point format " +
                                 std::to_string(h.point_format) + ")");
        if (!(h.channel_mask() & (1u << c)))
            return Status::error(StatusCode::InvalidArgument, "LAS: point format " + std::to_string(h.point_format) +
                                 " has no channel '" + name + "'");
        *mask |= 1u << c;
    }
    return Status::success();
}

}  // namespace las
}  // namespace pcr
