// las_header_san.cpp -- the LAS header parser (host/src/las_io.h) under AddressSanitizer + UBSan, on the CPU.  Given valid
// files (written by tests/las_common.py), every length and count field of the header and of the first variable length record
// is overwritten with 0, 1, all ones and the file size - 1, + 0, + 1, and the file is cut at every byte of the header and the
// first record.  The parser must answer every variant with a Status, and a header it accepts must describe bytes that exist.
// The record decoder then runs over exactly-sized heap buffers of every point format.
// Built and run by tests/test_las_io.py.
#include "las_io.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

namespace {

using Bytes = std::vector<unsigned char>;

long variants = 0, accepted = 0;

void fail(const std::string& what) {
    std::fprintf(stderr, "FAILED: %s\n", what.c_str());
    std::exit(1);
}

void parse(const std::string& path, const Bytes& data, const std::string& what) {
    {
        std::ofstream f(path, std::ios::binary | std::ios::trunc);
        f.write(reinterpret_cast<const char*>(data.data()), (std::streamsize)data.size());
    }
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) fail("cannot reopen " + path);
    pcr::las::Header h;
    const pcr::Status s = pcr::las::read_header(fd, path, &h);
    ::close(fd);
    ++variants;
    if (!s.ok()) {
        if (s.message.empty()) fail(what + ": an error without a message");
        return;
    }
    ++accepted;
    // what an accepted header promises
    if (h.file_size != data.size()) fail(what + ": file size");
    if (h.header_size < 227 || h.header_size > h.data_offset || h.data_offset > data.size()) fail(what + ": offsets outside the file");
    if (h.point_format < 0 || h.point_format > 10) fail(what + ": point format");
    if ((int)h.record_length < pcrhip::las::min_record_length(h.point_format)) fail(what + ": record length");
    if (h.num_points > (data.size() - h.data_offset) / h.record_length) fail(what + ": more points than bytes");
    unsigned mask = 0;
    if (!pcr::las::wanted_mask(h, {}, &mask).ok() || mask != h.channel_mask()) fail(what + ": channel mask");
}

void put(Bytes& b, size_t off, int width, unsigned long long v) {
    for (int k = 0; k < width && off + k < b.size(); ++k) b[off + k] = (unsigned char)(v >> (8 * k));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) fail("usage: las_header_san <scratch dir> <valid.las>...");
    const std::string scratch = std::string(argv[1]) + "/variant.las";
    for (int a = 2; a < argc; ++a) {
        std::ifstream in(argv[a], std::ios::binary);
        const Bytes good((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        const long before = accepted;
        parse(scratch, good, std::string(argv[a]) + " untouched");
        if (accepted != before + 1) fail(std::string(argv[a]) + ": the valid file was refused");
        const size_t header_size = good[94] | (good[95] << 8);
        const unsigned long long size = good.size();
        struct Field { size_t off; int width; };
        std::vector<Field> fields = {{94, 2}, {96, 4}, {100, 4}, {104, 1}, {105, 2}, {107, 4}};
        if (header_size >= 375) fields.push_back({247, 8});
        const bool has_vlr = (good[100] | good[101] | good[102] | good[103]) != 0;
        if (has_vlr) { fields.push_back({header_size + 18, 2}); fields.push_back({header_size + 20, 2}); }
        const unsigned long long values[] = {0ull, 1ull, ~0ull, size - 1, size, size + 1};
        for (const Field& f : fields)
            for (unsigned long long v : values) {
                Bytes b = good;
                put(b, f.off, f.width, v);
                parse(scratch, b, std::string(argv[a]) + " field @" + std::to_string(f.off) + " = " + std::to_string(v));
            }
        size_t cut_to = header_size;
        if (has_vlr && header_size + 54 <= good.size()) cut_to = header_size + 54 + (good[header_size + 20] | (good[header_size + 21] << 8));
        for (size_t t = 0; t <= cut_to + 1 && t <= good.size(); ++t)
            parse(scratch, Bytes(good.begin(), good.begin() + (long)t), std::string(argv[a]) + " cut at " + std::to_string(t));
    }
    // the record decoder (csrc/las_decode.hpp, compiled here for the host) on heap buffers of exactly n records: a read past
    // the last record, or before the first, is a sanitizer report
    for (int fmt = 0; fmt <= 10; ++fmt)
        for (int extra = 0; extra <= 1; ++extra) {
            pcr_hip_las_layout lay{};
            lay.point_format = fmt;
            lay.record_length = pcrhip::las::min_record_length(fmt) + extra;
            for (int k = 0; k < 3; ++k) { lay.scale[k] = 0.01; lay.offset[k] = 5.0; }
            const size_t n = 37;
            Bytes rec(n * (size_t)lay.record_length);
            for (size_t i = 0; i < rec.size(); ++i) rec[i] = (unsigned char)(i * 131 + fmt);
            double sum = 0.0;
            for (size_t i = 0; i < n; ++i) {
                const unsigned char* p = rec.data() + i * (size_t)lay.record_length;
                auto rd = [p](int o) -> unsigned { return p[o]; };
                auto put = [&sum](int, float v) { if (v > -1e30f && v < 1e30f) sum += v; };   // (the noise decodes to Inf / NaN GPS times too)
                double x, y;
                if (fmt >= 6) pcrhip::las::decode_record<true>(lay, pcrhip::las::channel_mask(fmt), rd, &x, &y, put);
                else pcrhip::las::decode_record<false>(lay, pcrhip::las::channel_mask(fmt), rd, &x, &y, put);
                sum += x + y;
            }
            if (!(sum == sum)) fail("decoder produced NaN coordinates");
        }
    std::printf("header parser survived %ld variants (%ld accepted)\n", variants, accepted);
    return 0;
}
