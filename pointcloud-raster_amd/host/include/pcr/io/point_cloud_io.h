// pcr/io/point_cloud_io.h -- point-cloud files either side of Pipeline::ingest (drop-in for the
// reference's include/pcr/io/point_cloud_io.h:14-99: same names, arguments and error behaviour).
//
// Native PCRP format (reference header, point_cloud_io.h:22-39), little-endian, packed:
//     u32 magic "PCRP" | u32 version = 1 | u64 num_points | u32 num_channels |
//     u32 crs_wkt_len | char crs_wkt[crs_wkt_len] |
//     { u16 name_len | char name[name_len] | u8 dtype (DataType) } x num_channels
//   body, SoA:  f64 x[num_points] | f64 y[num_points] | <dtype> channel[num_points] x num_channels
// CSV: header row "x,y,<channel>,...", values printed with 15 significant digits; every extra
// column is read back as Float64 (point_cloud_io.cpp:286-461).
//
// LAS input (not in the reference, which declares the format and leaves it NotImplemented): ASPRS LAS 1.0-1.4, point data
// record formats 0-10, little-endian.  x, y are Float64 ((double)X * scale + offset, one multiply and one add); every
// attribute the format has becomes a Float32 channel under laspy's name -- z, intensity, return_number, number_of_returns,
// classification, withheld, overlap, scan_angle (degrees), user_data, point_source_id, gps_time, red, green, blue, nir
// (include/pcr_hip.h: pcr_hip_las_decode holds the table).  Extra bytes and wave packets are skipped; the CRS comes from the
// OGC WKT record or the GeoKeyDirectory.  A file that starts with "LASF" is LAS whatever its extension.  A Device read ships
// the raw records over PCIe and unpacks them in HBM; Host reads run the same decoder on the CPU.  Writing LAS, and LAZ
// (compressed records) in either direction: NotImplemented, as upstream.
//
// Extensions (MI355X build): read_point_cloud can deliver the cloud in page-locked host memory or
// straight in HBM (`location`), and the streaming reader returns the right rows for every chunk --
// the reference's PCRP chunk reader advances through the SoA body as if it were AoS
// (point_cloud_io.cpp:575-612) and only returns valid data when one chunk covers the whole file.
#pragma once

#include "pcr/core/point_cloud.h"
#include "pcr/core/types.h"

#include <memory>
#include <string>
#include <vector>

namespace pcr {

enum class PointCloudFormat : uint8_t { PCR_Binary, CSV, LAS, LAZ, Auto };

struct PointCloudInfo {
    size_t num_points = 0;
    std::vector<ChannelDesc> channels;
    CRS crs;
    BBox bounds;                      // LAS: the header's min / max x, y; empty for PCRP and CSV, which do not store it
};

/// What a LAS read delivers.  channels: names from the list above, empty = every channel the file's point format has; an
/// unknown name or one the format lacks is InvalidArgument.  gps_time_origin is subtracted from the GPS time in Float64
/// before it is narrowed to the Float32 channel (GPS times are ~3e8 s, where Float32 resolves 32 s; over a flight of 1e4 s
/// it resolves 1 ms).
struct LasOptions {
    std::vector<std::string> channels;
    double gps_time_origin = 0.0;
};

/// Whole file -> PointCloud (nullptr on any failure, as upstream).  `location`: Host (default),
/// HostPinned (file read directly into page-locked memory) or Device (pinned staging, one H2D copy).
std::unique_ptr<PointCloud> read_point_cloud(const std::string& path,
                                             PointCloudFormat format = PointCloudFormat::Auto,
                                             MemoryLocation location = MemoryLocation::Host);

/// A LAS file with options; `status` (optional) says why nullptr was returned.
std::unique_ptr<PointCloud> read_las(const std::string& path, const LasOptions& options = LasOptions(),
                                     MemoryLocation location = MemoryLocation::Host, Status* status = nullptr);

Status read_point_cloud_info(const std::string& path, PointCloudInfo& info,
                             PointCloudFormat format = PointCloudFormat::Auto);

/// Cloud must be host-resident (Host or HostPinned).
Status write_point_cloud(const std::string& path, const PointCloud& cloud,
                         PointCloudFormat format = PointCloudFormat::PCR_Binary);

class PointCloudReader {
public:
    ~PointCloudReader();
    static std::unique_ptr<PointCloudReader> open(const std::string& path,
                                                  PointCloudFormat format = PointCloudFormat::Auto,
                                                  const LasOptions* las = nullptr, Status* status = nullptr);
    const PointCloudInfo& info() const;
    PointCloudFormat format() const;             // what the file turned out to be (never Auto)
    /// Next chunk of up to `max_points` into `cloud` (host-resident, capacity >= max_points; channels
    /// are added on first use).  Returns the number of points read, 0 at end of file.
    size_t read_chunk(PointCloud& cloud, size_t max_points);
    Status rewind();
    bool eof() const;

private:
    PointCloudReader() = default;
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

}  // namespace pcr
