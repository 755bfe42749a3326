// point_cloud_io.cpp -- PCRP / CSV / LAS point-cloud files (see pcr/io/point_cloud_io.h).
// Behaviour follows the reference's src/io/point_cloud_io.cpp (format detection :26-48, PCRP
// :75-283, CSV :291-461, dispatch :484-556, streaming reader :563-763); deliberate differences are
// listed in the header.  LAS input has no upstream counterpart: las_io.h reads the header block, pcr_hip_las_decode[_host]
// the records.
#include "pcr/io/point_cloud_io.h"

#include "buffer.h"
#include "las_io.h"

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <sstream>
#include <thread>

#include <fcntl.h>
#include <unistd.h>

namespace pcr {

namespace {

constexpr uint32_t kMagicPcrp = 0x50524350u;   // "PCRP"
constexpr uint32_t kMagicLasf = 0x4653414Cu;   // "LASF"
constexpr uint32_t kVersion = 1;

bool ends_with(const std::string& s, const std::string& suffix) {
    return s.size() >= suffix.size() && s.compare(s.size() - suffix.size(), suffix.size(), suffix) == 0;
}

std::string lower_case(const std::string& path) {
    std::string lower = path;
    std::transform(lower.begin(), lower.end(), lower.begin(), [](unsigned char c) { return (char)std::tolower(c); });
    return lower;
}

// a file that starts with "LASF" is LAS whatever it is called (a `.laz` name stays LAZ); then the extension
// (case-insensitive), then the PCRP magic number, then CSV
PointCloudFormat detect_format(const std::string& path) {
    const std::string lower = lower_case(path);
    if (ends_with(lower, ".laz")) return PointCloudFormat::LAZ;
    uint32_t magic = 0;
    {
        std::ifstream f(path, std::ios::binary);
        if (!f || !f.read(reinterpret_cast<char*>(&magic), 4)) magic = 0;
    }
    if (magic == kMagicLasf) return PointCloudFormat::LAS;
    if (ends_with(lower, ".pcrp")) return PointCloudFormat::PCR_Binary;
    if (ends_with(lower, ".csv")) return PointCloudFormat::CSV;
    if (ends_with(lower, ".las")) return PointCloudFormat::LAS;
    if (magic == kMagicPcrp) return PointCloudFormat::PCR_Binary;
    return PointCloudFormat::CSV;
}

bool host_resident(const PointCloud& c) {
    return c.location() == MemoryLocation::Host || c.location() == MemoryLocation::HostPinned;
}

bool known_dtype(uint8_t b) { return b <= static_cast<uint8_t>(DataType::UInt8); }

// ---- PCRP --------------------------------------------------------------------------------------
struct PcrpLayout {
    size_t header_bytes = 0;
    std::vector<size_t> channel_offset;          // byte offset of each channel's array in the file
    size_t x_offset = 0, y_offset = 0, file_bytes = 0;
};

Status read_pcrp_header(std::ifstream& ifs, const std::string& path, PointCloudInfo& info, PcrpLayout* lay) {
    if (!ifs) return Status::error(StatusCode::IoError, "failed to open file: " + path);
    uint32_t magic = 0, version = 0, num_channels = 0, wkt_len = 0;
    uint64_t num_points = 0;
    ifs.read(reinterpret_cast<char*>(&magic), 4);
    ifs.read(reinterpret_cast<char*>(&version), 4);
    ifs.read(reinterpret_cast<char*>(&num_points), 8);
    ifs.read(reinterpret_cast<char*>(&num_channels), 4);
    if (!ifs) return Status::error(StatusCode::IoError, "failed to read header");
    if (magic != kMagicPcrp) return Status::error(StatusCode::IoError, "invalid magic number (not a PCRP file)");
    if (version != kVersion) return Status::error(StatusCode::IoError, "unsupported version " + std::to_string(version));
    ifs.read(reinterpret_cast<char*>(&wkt_len), 4);
    if (!ifs || wkt_len > (1u << 24)) return Status::error(StatusCode::IoError, "failed to read header");
    std::string wkt(wkt_len, '\0');
    if (wkt_len) ifs.read(&wkt[0], wkt_len);
    std::vector<ChannelDesc> channels;
    size_t header = 4 + 4 + 8 + 4 + 4 + wkt_len;
    if (num_channels > 65536) return Status::error(StatusCode::IoError, "failed to read channel table");
    for (uint32_t i = 0; i < num_channels; ++i) {
        uint16_t name_len = 0;
        uint8_t dtype = 0;
        ifs.read(reinterpret_cast<char*>(&name_len), 2);
        std::string name(name_len, '\0');
        if (name_len) ifs.read(&name[0], name_len);
        ifs.read(reinterpret_cast<char*>(&dtype), 1);
        if (!ifs || !known_dtype(dtype)) return Status::error(StatusCode::IoError, "failed to read channel table");
        ChannelDesc d;
        d.name = name;
        d.dtype = static_cast<DataType>(dtype);
        channels.push_back(d);
        header += 2 + name_len + 1;
    }
    if (!ifs) return Status::error(StatusCode::IoError, "failed to read channel table");
    // the body the header declares must be there (a corrupt point count must not turn into a giant allocation)
    {
        const std::streampos here = ifs.tellg();
        ifs.seekg(0, std::ios::end);
        const uint64_t actual = (uint64_t)ifs.tellg();
        ifs.seekg(here);
        uint64_t row_bytes = 16;
        for (const auto& c : channels) row_bytes += data_type_size(c.dtype);
        if (actual < header || num_points > (actual - header) / row_bytes)
            return Status::error(StatusCode::IoError, "file is shorter than its header declares");
    }
    info.num_points = num_points;
    info.channels = channels;
    info.crs = CRS();
    info.crs.wkt = wkt;
    info.bounds = BBox();
    if (lay) {
        lay->header_bytes = header;
        lay->x_offset = header;
        lay->y_offset = header + num_points * 8;
        size_t off = header + num_points * 16;
        for (const auto& c : channels) {
            lay->channel_offset.push_back(off);
            off += num_points * data_type_size(c.dtype);
        }
        lay->file_bytes = off;
    }
    return Status::success();
}

Status write_pcrp(const std::string& path, const PointCloud& cloud) {
    if (!host_resident(cloud)) return Status::error(StatusCode::InvalidArgument, "cloud must be on host");
    std::ofstream ofs(path, std::ios::binary | std::ios::trunc);
    if (!ofs) return Status::error(StatusCode::IoError, "failed to open file for writing: " + path);
    const uint64_t n = cloud.count();
    const auto names = cloud.channel_names();
    const uint32_t magic = kMagicPcrp, version = kVersion, nch = (uint32_t)names.size();
    ofs.write(reinterpret_cast<const char*>(&magic), 4);
    ofs.write(reinterpret_cast<const char*>(&version), 4);
    ofs.write(reinterpret_cast<const char*>(&n), 8);
    ofs.write(reinterpret_cast<const char*>(&nch), 4);
    const std::string wkt = cloud.crs().wkt;
    const uint32_t wkt_len = (uint32_t)wkt.size();
    ofs.write(reinterpret_cast<const char*>(&wkt_len), 4);
    if (wkt_len) ofs.write(wkt.data(), wkt_len);
    for (const auto& name : names) {
        const ChannelDesc* d = cloud.channel(name);
        const uint16_t name_len = (uint16_t)name.size();
        const uint8_t dtype = static_cast<uint8_t>(d->dtype);
        ofs.write(reinterpret_cast<const char*>(&name_len), 2);
        ofs.write(name.data(), name_len);
        ofs.write(reinterpret_cast<const char*>(&dtype), 1);
    }
    if (!ofs) return Status::error(StatusCode::IoError, "failed to write header");
    if (n) {
        ofs.write(reinterpret_cast<const char*>(cloud.x()), n * sizeof(double));
        ofs.write(reinterpret_cast<const char*>(cloud.y()), n * sizeof(double));
        for (const auto& name : names) {
            const void* p = cloud.channel_data(name);
            if (!p) return Status::error(StatusCode::InvalidArgument, "failed to get channel data: " + name);
            ofs.write(static_cast<const char*>(p), n * data_type_size(cloud.channel(name)->dtype));
        }
    }
    if (!ofs) return Status::error(StatusCode::IoError, "failed to write point data");
    return Status::success();
}

// One array segment of the file -> memory.  Large reads are cut into pieces handled by a few threads: a single
// thread copying out of the page cache tops out near 6-11 GB/s, well under what the host-to-device link takes.
struct ReadSeg {
    char* dst;
    uint64_t offset;
    size_t bytes;
};

bool read_segments(int fd, const std::vector<ReadSeg>& segs) {
    constexpr size_t kPiece = 8u << 20;
    std::vector<ReadSeg> pieces;
    for (const ReadSeg& s : segs)
        for (size_t o = 0; o < s.bytes; o += kPiece) pieces.push_back({s.dst + o, s.offset + o, std::min(kPiece, s.bytes - o)});
    std::atomic<size_t> next{0};
    std::atomic<bool> ok{true};
    auto work = [&]() {
        for (size_t i = next++; i < pieces.size(); i = next++) {
            size_t done = 0;
            while (done < pieces[i].bytes) {
                const ssize_t r = ::pread(fd, pieces[i].dst + done, pieces[i].bytes - done, (off_t)(pieces[i].offset + done));
                if (r <= 0) { ok = false; return; }
                done += (size_t)r;
            }
        }
    };
    const size_t nthreads = std::min<size_t>({pieces.size(), 8, std::max(1u, std::thread::hardware_concurrency())});
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return ok;
}

// rows [first, first + count) of the file into the start of `cloud` (host-resident)
bool read_pcrp_rows(int fd, const PointCloudInfo& info, const PcrpLayout& lay, size_t first, size_t count,
                    PointCloud& cloud) {
    std::vector<ReadSeg> segs;
    segs.push_back({reinterpret_cast<char*>(cloud.x()), lay.x_offset + first * 8, count * 8});
    segs.push_back({reinterpret_cast<char*>(cloud.y()), lay.y_offset + first * 8, count * 8});
    for (size_t c = 0; c < info.channels.size(); ++c) {
        const ChannelDesc& ch = info.channels[c];
        if (!cloud.has_channel(ch.name) && !cloud.add_channel(ch.name, ch.dtype).ok()) return false;
        void* dst = cloud.channel_data(ch.name);
        const size_t es = data_type_size(ch.dtype);
        if (!dst || cloud.channel(ch.name)->dtype != ch.dtype) return false;
        segs.push_back({static_cast<char*>(dst), lay.channel_offset[c] + first * es, count * es});
    }
    return read_segments(fd, segs);
}

struct Fd {
    int fd = -1;
    explicit Fd(const std::string& path) : fd(::open(path.c_str(), O_RDONLY)) {}
    ~Fd() { if (fd >= 0) ::close(fd); }
    Fd(const Fd&) = delete;
    Fd& operator=(const Fd&) = delete;
};

std::unique_ptr<PointCloud> read_pcrp(const std::string& path, MemoryLocation location) {
    std::ifstream ifs(path, std::ios::binary);
    PointCloudInfo info;
    PcrpLayout lay;
    if (!read_pcrp_header(ifs, path, info, &lay).ok()) return nullptr;
    // host-side landing buffer: pageable for Host, page-locked otherwise (the H2D copy then runs at link speed)
    const MemoryLocation landing = location == MemoryLocation::Host ? MemoryLocation::Host : MemoryLocation::HostPinned;
    auto cloud = PointCloud::create(std::max<size_t>(info.num_points, 1), landing);
    if (!cloud) return nullptr;
    cloud->resize(info.num_points);
    cloud->set_crs(info.crs);
    for (const auto& ch : info.channels)
        if (!cloud->add_channel(ch.name, ch.dtype).ok()) return nullptr;
    Fd file(path);
    if (info.num_points && (file.fd < 0 || !read_pcrp_rows(file.fd, info, lay, 0, info.num_points, *cloud))) return nullptr;
    if (location == MemoryLocation::Device) return cloud->to(MemoryLocation::Device);
    return cloud;
}

// ---- CSV ---------------------------------------------------------------------------------------
Status write_csv(const std::string& path, const PointCloud& cloud) {
    if (!host_resident(cloud)) return Status::error(StatusCode::InvalidArgument, "cloud must be on host");
    std::ofstream ofs(path);
    if (!ofs) return Status::error(StatusCode::IoError, "failed to open file for writing: " + path);
    ofs << std::setprecision(15);
    const auto names = cloud.channel_names();
    ofs << "x,y";
    for (const auto& name : names) ofs << "," << name;
    ofs << "\n";
    for (const auto& name : names) {
        switch (cloud.channel(name)->dtype) {
            case DataType::Float32: case DataType::Float64: case DataType::Int32: case DataType::UInt32: break;
            default: return Status::error(StatusCode::InvalidArgument, "unsupported channel data type");
        }
    }
    for (size_t i = 0; i < cloud.count(); ++i) {
        ofs << cloud.x()[i] << "," << cloud.y()[i];
        for (const auto& name : names) {
            const void* p = cloud.channel_data(name);
            ofs << ",";
            switch (cloud.channel(name)->dtype) {
                case DataType::Float32: ofs << static_cast<const float*>(p)[i]; break;
                case DataType::Float64: ofs << static_cast<const double*>(p)[i]; break;
                case DataType::Int32: ofs << static_cast<const int32_t*>(p)[i]; break;
                default: ofs << static_cast<const uint32_t*>(p)[i]; break;
            }
        }
        ofs << "\n";
    }
    if (!ofs) return Status::error(StatusCode::IoError, "failed to write CSV data");
    return Status::success();
}

size_t count_csv_rows(const std::string& path) {
    std::ifstream f(path);
    size_t lines = 0;
    std::string line;
    while (std::getline(f, line)) ++lines;
    return lines > 0 ? lines - 1 : 0;
}

Status read_csv_info(const std::string& path, PointCloudInfo& info) {
    std::ifstream ifs(path);
    if (!ifs) return Status::error(StatusCode::IoError, "failed to open file: " + path);
    std::string header;
    if (!std::getline(ifs, header)) return Status::error(StatusCode::IoError, "empty CSV file");
    if (!header.empty() && header.back() == '\r') header.pop_back();
    std::vector<std::string> cols;
    std::istringstream hs(header);
    std::string tok;
    while (std::getline(hs, tok, ',')) cols.push_back(tok);
    if (cols.size() < 2 || cols[0] != "x" || cols[1] != "y")
        return Status::error(StatusCode::IoError, "CSV must start with x,y columns");
    info.channels.clear();
    for (size_t i = 2; i < cols.size(); ++i) {
        ChannelDesc d;
        d.name = cols[i];
        d.dtype = DataType::Float64;                 // as upstream: every extra column is read as f64
        info.channels.push_back(d);
    }
    info.num_points = count_csv_rows(path);
    info.crs = CRS();
    info.bounds = BBox();
    return Status::success();
}

// one data row -> x, y, channel values; false on a malformed row (upstream lets std::stod throw)
bool parse_csv_row(const std::string& line, size_t nch, double& x, double& y, std::vector<double>& ch) {
    std::istringstream ls(line);
    std::string tok;
    try {
        if (!std::getline(ls, tok, ',')) return false;
        x = std::stod(tok);
        if (!std::getline(ls, tok, ',')) return false;
        y = std::stod(tok);
        for (size_t c = 0; c < nch; ++c) {
            if (!std::getline(ls, tok, ',')) return false;
            ch[c] = std::stod(tok);
        }
    } catch (const std::exception&) {
        return false;
    }
    return true;
}

// up to max_rows rows from the stream into the start of `cloud`; returns rows read
size_t read_csv_rows(std::ifstream& ifs, const PointCloudInfo& info, size_t max_rows, PointCloud& cloud) {
    for (const auto& ch : info.channels)
        if (!cloud.has_channel(ch.name) && !cloud.add_channel(ch.name, ch.dtype).ok()) return 0;
    std::vector<double*> dst;
    for (const auto& ch : info.channels) {
        const ChannelDesc* d = cloud.channel(ch.name);
        dst.push_back(d && d->dtype == DataType::Float64 ? static_cast<double*>(cloud.channel_data(ch.name)) : nullptr);
    }
    std::vector<double> vals(info.channels.size());
    std::string line;
    size_t n = 0;
    while (n < max_rows && std::getline(ifs, line)) {
        double x, y;
        if (!parse_csv_row(line, vals.size(), x, y, vals)) break;
        cloud.x()[n] = x;
        cloud.y()[n] = y;
        for (size_t c = 0; c < vals.size(); ++c)
            if (dst[c]) dst[c][n] = vals[c];
        ++n;
    }
    return n;
}

std::unique_ptr<PointCloud> read_csv(const std::string& path, MemoryLocation location) {
    PointCloudInfo info;
    if (!read_csv_info(path, info).ok()) return nullptr;
    std::ifstream ifs(path);
    if (!ifs) return nullptr;
    std::string header;
    std::getline(ifs, header);
    const MemoryLocation landing = location == MemoryLocation::Host ? MemoryLocation::Host : MemoryLocation::HostPinned;
    auto cloud = PointCloud::create(std::max<size_t>(info.num_points, 1), landing);
    if (!cloud) return nullptr;
    cloud->resize(info.num_points);
    cloud->set_crs(info.crs);
    const size_t n = read_csv_rows(ifs, info, info.num_points, *cloud);
    cloud->resize(n);
    if (location == MemoryLocation::Device) return cloud->to(MemoryLocation::Device);
    return cloud;
}

const char* kLasMessage = "LAS/LAZ format support not yet implemented";     // writing LAS; LAZ either way

// ---- LAS ---------------------------------------------------------------------------------------
struct LasFile {
    std::unique_ptr<Fd> file;
    las::Header header;
    unsigned want = 0;                           // PCR_HIP_LAS_CH_* bits delivered
    pcr_hip_las_layout layout{};
};

Status open_las(const std::string& path, const LasOptions& options, LasFile* out) {
    if (ends_with(lower_case(path), ".laz")) return Status::error(StatusCode::NotImplemented, las::kLazMessage);
    out->file = std::make_unique<Fd>(path);
    if (out->file->fd < 0)
        return Status::error(StatusCode::IoError, "failed to open LAS file: " + path + " (note: LAZ support not yet implemented)");
    Status s = las::read_header(out->file->fd, path, &out->header);
    if (s.ok()) s = las::wanted_mask(out->header, options.channels, &out->want);
    out->layout = out->header.layout(options.gps_time_origin);
    return s;
}

void las_info(const LasFile& f, PointCloudInfo& info) {
    info.num_points = (size_t)f.header.num_points;
    info.channels.clear();
    for (int c = 0; c < PCR_HIP_LAS_CH_COUNT; ++c) {
        if (!(f.want & (1u << c))) continue;
        ChannelDesc d;
        d.name = las::kChannelNames[c];
        d.dtype = DataType::Float32;
        info.channels.push_back(d);
    }
    info.crs = f.header.crs;
    info.bounds = f.header.bounds;
}

// The cloud's arrays for the wanted channels (added on first use), `at` elements in.
Status las_outputs(const LasFile& f, PointCloud& cloud, size_t at, float** out) {
    for (int c = 0; c < PCR_HIP_LAS_CH_COUNT; ++c) {
        out[c] = nullptr;
        if (!(f.want & (1u << c))) continue;
        const std::string name = las::kChannelNames[c];
        if (!cloud.has_channel(name)) {
            Status s = cloud.add_channel(name, DataType::Float32);
            if (!s.ok()) return s;
        }
        const ChannelDesc* d = cloud.channel(name);
        if (!d || d->dtype != DataType::Float32 || !cloud.channel_f32(name))
            return Status::error(StatusCode::InvalidArgument, "LAS: channel '" + name + "' of the cloud is not Float32");
        out[c] = cloud.channel_f32(name) + at;
    }
    return Status::success();
}

int las_host_threads() { return (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency())); }

// records [first, first + count) -> elements [at, at + count) of a host-resident cloud, through `raw` (grown as needed)
Status las_rows_to_host(const LasFile& f, size_t first, size_t count, PointCloud& cloud, size_t at, std::vector<uint8_t>& raw) {
    float* out[PCR_HIP_LAS_CH_COUNT];
    Status s = las_outputs(f, cloud, at, out);
    if (!s.ok() || count == 0) return s;
    const size_t len = f.header.record_length;
    if (raw.size() < count * len) raw.resize(count * len);
    if (!read_segments(f.file->fd, {{reinterpret_cast<char*>(raw.data()), f.header.data_offset + (uint64_t)first * len, count * len}}))
        return Status::error(StatusCode::IoError, "LAS: failed to read point records");
    return detail::hip_status(pcr_hip_las_decode_host(&f.layout, raw.data(), count, cloud.x() + at, cloud.y() + at, out, las_host_threads()));
}

std::unique_ptr<PointCloud> read_las_file(const std::string& path, const LasOptions& options, MemoryLocation location, Status* status) {
    Status unused;
    Status& st = status ? *status : unused;
    LasFile f;
    if (!(st = open_las(path, options, &f)).ok()) return nullptr;
    const size_t n = (size_t)f.header.num_points, len = f.header.record_length;
    auto cloud = PointCloud::create(std::max<size_t>(n, 1), location);
    if (!cloud) { st = Status::error(StatusCode::OutOfMemory, "LAS: failed to allocate the point cloud"); return nullptr; }
    cloud->resize(n);
    cloud->set_crs(f.header.crs);
    if (location != MemoryLocation::Device) {
        // in pieces, so that the raw records never take more than 8 M points' worth of memory beside the cloud
        constexpr size_t kPiece = 8u << 20;
        std::vector<uint8_t> raw;
        if (n == 0) st = las_rows_to_host(f, 0, 0, *cloud, 0, raw);
        for (size_t first = 0; first < n && st.ok(); first += kPiece)
            st = las_rows_to_host(f, first, std::min(kPiece, n - first), *cloud, first, raw);
        if (!st.ok()) return nullptr;
        return cloud;
    }
    // Device: the raw records cross PCIe once, out of a page-locked buffer, and are unpacked in HBM
    float* out[PCR_HIP_LAS_CH_COUNT];
    if (!(st = las_outputs(f, *cloud, 0, out)).ok()) return nullptr;
    if (n == 0) return cloud;
    detail::Buffer pinned, d_records;
    const size_t bytes = n * len;
    if (!(st = pinned.allocate(bytes + 16, MemoryLocation::HostPinned)).ok()) return nullptr;
    if (!(st = d_records.allocate(bytes + 16, MemoryLocation::Device)).ok()) return nullptr;
    if (!read_segments(f.file->fd, {{static_cast<char*>(pinned.data()), f.header.data_offset, bytes}})) {
        st = Status::error(StatusCode::IoError, "LAS: failed to read point records");
        return nullptr;
    }
    std::memset(static_cast<char*>(pinned.data()) + bytes, 0, 16);
    if (!(st = detail::hip_status(pcr_hip_memcpy_h2d(d_records.data(), pinned.data(), bytes + 16, nullptr))).ok()) return nullptr;
    if (!(st = detail::hip_status(pcr_hip_las_decode(&f.layout, static_cast<const uint8_t*>(d_records.data()), n, cloud->x(),
                                                     cloud->y(), out, nullptr))).ok()) return nullptr;
    if (!(st = detail::hip_status(pcr_hip_stream_synchronize(nullptr))).ok()) return nullptr;
    return cloud;
}

}  // namespace

// ---- public API ----------------------------------------------------------------------------------
std::unique_ptr<PointCloud> read_point_cloud(const std::string& path, PointCloudFormat format, MemoryLocation location) {
    if (format == PointCloudFormat::Auto) format = detect_format(path);
    switch (format) {
        case PointCloudFormat::PCR_Binary: return read_pcrp(path, location);
        case PointCloudFormat::CSV: return read_csv(path, location);
        case PointCloudFormat::LAS: return read_las_file(path, LasOptions(), location, nullptr);
        default: return nullptr;                              // LAZ: not implemented upstream either
    }
}

std::unique_ptr<PointCloud> read_las(const std::string& path, const LasOptions& options, MemoryLocation location, Status* status) {
    return read_las_file(path, options, location, status);
}

Status read_point_cloud_info(const std::string& path, PointCloudInfo& info, PointCloudFormat format) {
    if (format == PointCloudFormat::Auto) format = detect_format(path);
    switch (format) {
        case PointCloudFormat::PCR_Binary: {
            std::ifstream ifs(path, std::ios::binary);
            return read_pcrp_header(ifs, path, info, nullptr);
        }
        case PointCloudFormat::CSV: return read_csv_info(path, info);
        case PointCloudFormat::LAS: {
            LasFile f;
            Status s = open_las(path, LasOptions(), &f);
            if (s.ok()) las_info(f, info);
            return s;
        }
        case PointCloudFormat::LAZ: return Status::error(StatusCode::NotImplemented, kLasMessage);
        default: return Status::error(StatusCode::InvalidArgument, "unknown format");
    }
}

Status write_point_cloud(const std::string& path, const PointCloud& cloud, PointCloudFormat format) {
    if (format == PointCloudFormat::Auto) format = detect_format(path);
    switch (format) {
        case PointCloudFormat::PCR_Binary: return write_pcrp(path, cloud);
        case PointCloudFormat::CSV: return write_csv(path, cloud);
        case PointCloudFormat::LAS:
        case PointCloudFormat::LAZ: return Status::error(StatusCode::NotImplemented, kLasMessage);
        default: return Status::error(StatusCode::InvalidArgument, "unknown format");
    }
}

// ---- streaming reader ------------------------------------------------------------------------------
struct PointCloudReader::Impl {
    std::ifstream file;
    PointCloudInfo info;
    PcrpLayout layout;
    PointCloudFormat format = PointCloudFormat::Auto;
    size_t points_read = 0;
    std::unique_ptr<Fd> raw;                     // PCRP body reads (pread, position-independent)
    LasFile las;                                 // LAS: the open file, its header and the wanted channels
    std::vector<uint8_t> las_raw;                // LAS: one chunk of records, as read
    bool is_open() const { return format == PointCloudFormat::LAS ? las.file != nullptr : file.is_open(); }
};

PointCloudReader::~PointCloudReader() = default;

std::unique_ptr<PointCloudReader> PointCloudReader::open(const std::string& path, PointCloudFormat format, const LasOptions* las,
                                                         Status* status) {
    Status unused;
    Status& st = status ? *status : unused;
    st = Status::error(StatusCode::IoError, "");
    if (format == PointCloudFormat::Auto) format = detect_format(path);
    auto r = std::unique_ptr<PointCloudReader>(new PointCloudReader());
    r->impl_ = std::make_unique<Impl>();
    r->impl_->format = format;
    if (format == PointCloudFormat::PCR_Binary) {
        r->impl_->file.open(path, std::ios::binary);
        if (!read_pcrp_header(r->impl_->file, path, r->impl_->info, &r->impl_->layout).ok()) return nullptr;
        r->impl_->raw = std::make_unique<Fd>(path);
        if (r->impl_->raw->fd < 0) return nullptr;
    } else if (format == PointCloudFormat::CSV) {
        if (!read_csv_info(path, r->impl_->info).ok()) return nullptr;
        r->impl_->file.open(path);
        if (!r->impl_->file) return nullptr;
        std::string header;
        std::getline(r->impl_->file, header);
    } else if (format == PointCloudFormat::LAS) {
        if (!(st = open_las(path, las ? *las : LasOptions(), &r->impl_->las)).ok()) return nullptr;
        las_info(r->impl_->las, r->impl_->info);
    } else {
        if (format == PointCloudFormat::LAZ) st = Status::error(StatusCode::NotImplemented, kLasMessage);
        return nullptr;
    }
    st = Status::success();
    return r;
}

const PointCloudInfo& PointCloudReader::info() const { return impl_->info; }
PointCloudFormat PointCloudReader::format() const { return impl_->format; }

size_t PointCloudReader::read_chunk(PointCloud& cloud, size_t max_points) {
    if (!impl_ || !impl_->is_open() || !host_resident(cloud)) return 0;
    Impl& s = *impl_;
    if (s.format == PointCloudFormat::LAS) {                     // a contiguous pread of whole records, decoded on the host
        if (s.points_read >= s.info.num_points) return 0;
        const size_t n = std::min(max_points, s.info.num_points - s.points_read);
        if (!cloud.resize(n).ok()) return 0;
        if (!las_rows_to_host(s.las, s.points_read, n, cloud, 0, s.las_raw).ok()) return 0;
        s.points_read += n;
        return n;
    }
    if (s.format == PointCloudFormat::PCR_Binary) {
        if (s.points_read >= s.info.num_points) return 0;
        const size_t n = std::min(max_points, s.info.num_points - s.points_read);
        if (!cloud.resize(n).ok()) return 0;
        if (!read_pcrp_rows(s.raw->fd, s.info, s.layout, s.points_read, n, cloud)) return 0;
        s.points_read += n;
        return n;
    }
    if (!cloud.resize(max_points).ok()) return 0;
    const size_t n = read_csv_rows(s.file, s.info, max_points, cloud);
    cloud.resize(n);
    s.points_read += n;
    return n;
}

Status PointCloudReader::rewind() {
    if (!impl_ || !impl_->is_open()) return Status::error(StatusCode::InvalidArgument, "reader not open");
    impl_->points_read = 0;
    if (impl_->format == PointCloudFormat::LAS) return Status::success();
    impl_->file.clear();
    impl_->file.seekg(0, std::ios::beg);
    if (impl_->format == PointCloudFormat::CSV) {
        std::string header;
        std::getline(impl_->file, header);
    }
    return Status::success();
}

bool PointCloudReader::eof() const { return !impl_ || impl_->points_read >= impl_->info.num_points; }

}  // namespace pcr
