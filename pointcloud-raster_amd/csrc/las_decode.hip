// las_decode.hip -- pcr_hip_las_decode / pcr_hip_las_decode_host (include/pcr_hip.h): LAS point records -> x, y and the
// Float32 channels.  The device kernel and its host twin are both built from las_decode.hpp.
//
// The input is array-of-structures with a record stride of 20-70 bytes that is rarely a multiple of 16, so a lane that
// read its own record from HBM would issue unaligned loads that split cache lines.  Instead a workgroup owns a run of
// consecutive records, copies the run's byte range into LDS with aligned 16-byte loads (every byte of it belongs to some
// lane's record), and each lane then picks its fields out of LDS with byte reads; the outputs are one f64 / f32 per lane
// per wanted array: coalesced in, coalesced out.  LDS bank behaviour of the byte reads: DESIGN.md section 15.
#include "common.hpp"
#include "las_decode.hpp"

#include <algorithm>
#include <thread>
#include <vector>

namespace pcrhip {
namespace {

constexpr int kBlock = 256;
constexpr int kPasses = PCR_HIP_LAS_RECORDS_PER_LANE;      // a workgroup's run: kPasses x kBlock records, one LDS tile at a time
constexpr int kTileBytes = 32768;
// 256 records + the up to 15 bytes in front of the first and behind the last must fit the tile: 256 * 126 + 30 <= 32768.
// Longer records (no such file is known) are read straight from memory, uncoalesced but correct.
constexpr int kMaxStagedLength = 126;

struct Outs {
    double* x;
    double* y;
    float* ch[PCR_HIP_LAS_CH_COUNT];
};

struct ByteReader {
    const uint8_t* p;
    PCR_HD unsigned operator()(int o) const { return p[o]; }
};

struct Put {
    const Outs* o;
    uint64_t i;
    PCR_HD void operator()(int c, float v) const { o->ch[c][i] = v; }
};

template <bool NEW>
__global__ void __launch_bounds__(kBlock) k_las_decode(pcr_hip_las_layout lay, const uint8_t* __restrict__ rec, uint64_t n, Outs o,
                                                       unsigned want) {
    __shared__ uint4 tile[kTileBytes / 16];
    const unsigned len = (unsigned)lay.record_length;
    const uint64_t run0 = (uint64_t)blockIdx.x * (kBlock * kPasses);
    for (int pass = 0; pass < kPasses; ++pass) {
        const uint64_t first = run0 + (uint64_t)pass * kBlock;
        if (first >= n) break;                                              // uniform
        const unsigned cnt = (unsigned)min((uint64_t)kBlock, n - first);
        const uint64_t b0 = first * len, b1 = b0 + (uint64_t)cnt * len;    // the run's bytes
        const uint64_t a0 = b0 & ~(uint64_t)15;                             // rec is 16-byte aligned: a0 >= 0 stays inside it
        const unsigned chunks = (unsigned)((((b1 + 15) & ~(uint64_t)15) - a0) >> 4);   // <= (256 * 126 + 30) / 16 < 2048
        const uint4* src = reinterpret_cast<const uint4*>(rec + a0);
        for (unsigned c = threadIdx.x; c < chunks; c += kBlock) tile[c] = stream_load(src + c);
        __syncthreads();
        if (threadIdx.x < cnt) {
            const ByteReader rd{reinterpret_cast<const uint8_t*>(tile) + (unsigned)(b0 - a0) + threadIdx.x * len};
            const uint64_t i = first + threadIdx.x;
            double x, y;
            las::decode_record<NEW>(lay, want, rd, &x, &y, Put{&o, i});
            o.x[i] = x;
            o.y[i] = y;
        }
        __syncthreads();                                                    // the tile is overwritten by the next pass
    }
}

template <bool NEW>
__global__ void __launch_bounds__(kBlock) k_las_decode_long(pcr_hip_las_layout lay, const uint8_t* __restrict__ rec, uint64_t n, Outs o,
                                                            unsigned want) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const ByteReader rd{rec + i * (uint64_t)lay.record_length};
    double x, y;
    las::decode_record<NEW>(lay, want, rd, &x, &y, Put{&o, i});
    o.x[i] = x;
    o.y[i] = y;
}

// What both entry points check, before anything else happens.
int check_args(const char* who, const pcr_hip_las_layout* lay, const uint8_t* records, uint64_t n, double* x, double* y,
               float* const* channels, Outs* o, unsigned* want) {
    const std::string w(who);
    PCR_REQUIRE(lay, w + ": null layout");
    PCR_REQUIRE(lay->point_format >= 0 && lay->point_format <= las::kMaxFormat,
                w + ": point format " + std::to_string(lay->point_format) + " is not supported (0-10)");
    PCR_REQUIRE(lay->record_length >= las::min_record_length(lay->point_format) && lay->record_length <= 65535,
                w + ": record_length " + std::to_string(lay->record_length) + " is outside " +
                std::to_string(las::min_record_length(lay->point_format)) + "..65535 for point format " + std::to_string(lay->point_format));
    *want = 0u;
    *o = Outs{};
    const unsigned have = las::channel_mask(lay->point_format);
    for (int c = 0; channels && c < PCR_HIP_LAS_CH_COUNT; ++c) {
        if (!channels[c]) continue;
        PCR_REQUIRE(have & (1u << c), w + ": channel " + std::to_string(c) + " is wanted but point format " +
                                      std::to_string(lay->point_format) + " does not have it");
        *want |= 1u << c;
        o->ch[c] = channels[c];
    }
    if (n == 0) return PCR_HIP_OK;
    PCR_REQUIRE(x && y, w + ": null x or y array");
    PCR_REQUIRE(records, w + ": null record buffer");
    o->x = x;
    o->y = y;
    return PCR_HIP_OK;
}

template <bool NEW>
void decode_host_range(const pcr_hip_las_layout& lay, const uint8_t* rec, uint64_t i0, uint64_t i1, const Outs& o, unsigned want) {
    for (uint64_t i = i0; i < i1; ++i) {
        const ByteReader rd{rec + i * (uint64_t)lay.record_length};
        las::decode_record<NEW>(lay, want, rd, o.x + i, o.y + i, Put{&o, i});
    }
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" {

int pcr_hip_las_decode(const pcr_hip_las_layout* layout, const uint8_t* d_records, uint64_t n, double* d_x, double* d_y,
                       float* const* channels, pcr_hip_stream s) {
    Outs o;
    unsigned want = 0u;
    const int rc = check_args("las_decode", layout, d_records, n, d_x, d_y, channels, &o, &want);
    if (rc != PCR_HIP_OK || n == 0) return rc;
    PCR_REQUIRE((reinterpret_cast<uintptr_t>(d_records) & 15) == 0, "las_decode: the record buffer must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(s);
    const bool is_new = layout->point_format >= 6;
    const bool staged = layout->record_length <= kMaxStagedLength;
    const uint64_t per_block = staged ? (uint64_t)kBlock * kPasses : (uint64_t)kBlock;
    const uint64_t blocks = (n + per_block - 1) / per_block;
    PCR_REQUIRE(blocks <= 0x7FFFFFFFull, "las_decode: more than 2^31 workgroups");
    const dim3 grid((unsigned)blocks), block(kBlock);
    if (staged) {
        if (is_new) hipLaunchKernelGGL(k_las_decode<true>, grid, block, 0, st, *layout, d_records, n, o, want);
        else hipLaunchKernelGGL(k_las_decode<false>, grid, block, 0, st, *layout, d_records, n, o, want);
    } else {
        if (is_new) hipLaunchKernelGGL(k_las_decode_long<true>, grid, block, 0, st, *layout, d_records, n, o, want);
        else hipLaunchKernelGGL(k_las_decode_long<false>, grid, block, 0, st, *layout, d_records, n, o, want);
    }
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

int pcr_hip_las_decode_host(const pcr_hip_las_layout* layout, const uint8_t* h_records, uint64_t n, double* h_x, double* h_y,
                            float* const* channels, int threads) {
    Outs o;
    unsigned want = 0u;
    const int rc = check_args("las_decode_host", layout, h_records, n, h_x, h_y, channels, &o, &want);
    if (rc != PCR_HIP_OK || n == 0) return rc;
    const pcr_hip_las_layout lay = *layout;
    const bool is_new = lay.point_format >= 6;
    auto range = [&](uint64_t i0, uint64_t i1) {
        if (is_new) decode_host_range<true>(lay, h_records, i0, i1, o, want);
        else decode_host_range<false>(lay, h_records, i0, i1, o, want);
    };
    // contiguous parts, one per thread; a part below 4 K records is not worth a thread of its own
    const uint64_t parts = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), (n + 4095) / 4096));
    if (parts == 1) { range(0, n); return PCR_HIP_OK; }
    const uint64_t per = (n + parts - 1) / parts;
    std::vector<std::thread> pool;
    for (uint64_t p = 1; p < parts; ++p) pool.emplace_back(range, std::min(n, p * per), std::min(n, (p + 1) * per));
    range(0, std::min(n, per));
    for (auto& t : pool) t.join();
    return PCR_HIP_OK;
}

}  // extern "C"
