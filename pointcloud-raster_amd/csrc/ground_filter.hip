// ground_filter.hip -- pcr_hip_ground_filter: a progressive morphological filter on one band (the contract: ground_filter.hpp),
// out of place, and pcr_hip_band_difference.
//
// A level is four passes over planes of the workspace: row-erode, column-erode, row-dilate, column-dilate.  Every pass is the
// same machine.  One wave (a workgroup of 64 lanes) owns a tile of 64 LINES x 64 cells along the pass's axis -- for a row pass
// the lines are 64 image rows, for a column pass 64 image columns -- and
//   1  stages the tile with an apron of R cells at both ends of every line in LDS: 16-byte loads, eight of them in flight per
//      lane, every wave access a row segment (a column pass reads four 64-cell row segments per instruction), cells outside
//      the image as NaN;
//   2  every lane takes ONE line and evaluates its 64 windows of 2R + 1 cells in place with ground::line_window (R <= 4: the
//      window is walked; beyond: van Herk / Gil-Werman, three LDS accesses and two v_min / v_max per staged cell whatever R
//      is; either way in groups of eight cells, loads before stores, one LDS round trip per group).  A row pass keeps the
//      lines 64 + 2R + 1 floats apart, an odd pitch, a column pass 64 floats apart with the lane as the column: either way the
//      64 lanes of an access hit 64 different banks;
//   3  stores the 64 x 64 results with 16-byte stores, rows again.
// The first pass of level 1 reads src and also stores dst = src (NaNs as 0x7FC00000), so dst costs no pass of its own.  The
// column-dilate pass holds Ok in LDS when it stores: it reads A(k-1) at the cells it owns, stores 0x7FC00000 into dst where
// A(k-1) - Ok > tk -- dst(c) is not NaN exactly while c is still ground, the verdict needs no plane -- and stores Ok over
// A(k-1), which nobody else reads.  Workspace: A and two temporaries, three planes with rows padded to whole quads.
// LDS is dynamic, sized by R: 64 x (64 + 2R [+ 1]) floats = 17 KB at R = 1, 24 KB at R = 16, 48 KB at R = 64, so the waves a CU
// holds fall from 9 to 3 as the apron grows.  No atomics, no scratch.  Measured: profiles/ground_filter.md.
#include "band_pass.hpp"
#include "ground_filter.hpp"

namespace pcrhip {
namespace {

using namespace ground;
using band::aligned16;
using band::load_quad;

constexpr int kLines = 64;                                       // lines of a tile = lanes of its wave
constexpr int kTile = 64;                                        // cells of a tile along the pass's axis
constexpr int kBatch = 8;                                        // global loads a lane keeps in flight while it stages

struct PassArgs {
    const float* in;                 // the plane the windows are taken of
    float* out;                      // a workspace plane (rows start on 16 bytes, padded to whole quads); null: not stored
    const float* a_in;               // column-dilate: A(k-1)
    float* dst;                      // row-erode of level 1: receives the cleaned copy of `in`; column-dilate: receives the verdicts
    int w, h;
    int64_t in_stride, out_stride, a_stride, dst_stride;
    int R;
    float t;
    int a_vec, dst_vec;              // a_in / dst rows start on 16 bytes
};

__device__ __forceinline__ int pad4(int R) { return (R + 3) & ~3; }

// ---- a row pass: the tile's lines are image rows r0 .. r0 + 63, its cells columns c0 .. c0 + 63
template <bool MAX, bool VEC>                                    // VEC: the rows of `in` start on 16 bytes
__global__ __launch_bounds__(kLines) void k_ground_rows(const PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int R = a.R, Ra = pad4(R);
    const int quads = (kTile + 2 * Ra) / 4, pitch = kTile + 2 * Ra + 1;
    const int c0 = blockIdx.x * kTile, r0 = blockIdx.y * kLines;

    // 1: LDS column i of a line is image column c0 - Ra + i.  kBatch loads are issued before the first of them is waited for.
    const int items = quads * kLines;
    for (int base = lane; base < items; base += kBatch * kLines) {
        float4 x[kBatch];
        PCR_GF_UNROLL
        for (int u = 0; u < kBatch; ++u) {
            const int i = base + u * kLines;
            const int rr = i / quads, q = i - rr * quads;
            const int r = r0 + rr;
            x[u] = load_quad<VEC>(i < items && r < a.h ? a.in + (int64_t)r * a.in_stride : nullptr, c0 - Ra + 4 * q, a.w);
        }
        PCR_GF_UNROLL
        for (int u = 0; u < kBatch; ++u) {
            const int i = base + u * kLines;
            if (i >= items) continue;
            const int rr = i / quads, q = i - rr * quads;
            const int r = r0 + rr, c = c0 - Ra + 4 * q;
            const float4 y = make_float4(clean(x[u].x), clean(x[u].y), clean(x[u].z), clean(x[u].w));
            float* l = lds + rr * pitch + 4 * q;
            l[0] = y.x; l[1] = y.y; l[2] = y.z; l[3] = y.w;
            if (a.dst && r < a.h && c >= c0 && c < c0 + kTile && c < a.w) {
                float* d = a.dst + (int64_t)r * a.dst_stride + c;
                if (a.dst_vec && c + 4 <= a.w) {
                    *reinterpret_cast<pcr_f4v*>(d) = pcr_f4v{y.x, y.y, y.z, y.w};
                } else {
                    d[0] = y.x;
                    if (c + 1 < a.w) d[1] = y.y;
                    if (c + 2 < a.w) d[2] = y.z;
                    if (c + 3 < a.w) d[3] = y.w;
                }
            }
        }
    }
    __syncthreads();
    // 2: the line's first wanted cell is column c0, R cells into the apron
    line_window<MAX>(lds + lane * pitch + (Ra - R), 1, R, kTile);
    __syncthreads();
    // 3: (a quad that starts inside the row may end in its padding)
    for (int i = lane; i < kLines * (kTile / 4); i += kLines) {
        const int rr = i / (kTile / 4), q = i % (kTile / 4);
        const int r = r0 + rr, c = c0 + 4 * q;
        if (r >= a.h || c >= a.w) continue;
        const float* l = lds + rr * pitch + (Ra - R) + 4 * q;
        *reinterpret_cast<pcr_f4v*>(a.out + (int64_t)r * a.out_stride + c) = pcr_f4v{l[0], l[1], l[2], l[3]};
    }
}

// ---- a column pass: the tile's lines are image columns c0 .. c0 + 63, its cells rows r0 .. r0 + 63.  `in` is a workspace plane.
template <bool MAX, bool TEST>
__global__ __launch_bounds__(kLines) void k_ground_cols(const PassArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int R = a.R;
    const int c0 = blockIdx.x * kLines, r0 = blockIdx.y * kTile;
    constexpr int kQ = kLines / 4;

    // 1: LDS row i is image row r0 - R + i.  kBatch loads are issued before the first of them is waited for.
    const int items = (kTile + 2 * R) * kQ;
    for (int base = lane; base < items; base += kBatch * kLines) {
        float4 x[kBatch];
        PCR_GF_UNROLL
        for (int u = 0; u < kBatch; ++u) {
            const int i = base + u * kLines;
            const int r = r0 - R + i / kQ;
            x[u] = load_quad<true>(i < items && r >= 0 && r < a.h ? a.in + (int64_t)r * a.in_stride : nullptr, c0 + 4 * (i % kQ), a.w);
        }
        PCR_GF_UNROLL
        for (int u = 0; u < kBatch; ++u) {
            const int i = base + u * kLines;
            if (i < items) *reinterpret_cast<float4*>(lds + (i / kQ) * kLines + 4 * (i % kQ)) = x[u];
        }
    }
    __syncthreads();
    line_window<MAX>(lds + lane, kLines, R, kTile);
    __syncthreads();
    // 3: (kTile * kQ is a whole number of batches; a column-dilate pass reads A(k-1) a batch at a time too)
    for (int base = lane; base < kTile * kQ; base += kBatch * kLines) {
        float4 A[kBatch];
        if (TEST) {
            PCR_GF_UNROLL
            for (int u = 0; u < kBatch; ++u) {
                const int i = base + u * kLines;
                const int r = r0 + i / kQ, c = c0 + 4 * (i % kQ);
                A[u] = load_quad(r < a.h && c < a.w ? a.a_in + (int64_t)r * a.a_stride : nullptr, c, a.w, a.a_vec);
            }
        }
        PCR_GF_UNROLL
        for (int u = 0; u < kBatch; ++u) {
            const int i = base + u * kLines;
            const int rr = i / kQ, q = i % kQ;
            const int r = r0 + rr, c = c0 + 4 * q;
            if (r >= a.h || c >= a.w) continue;
            const float4 o = *reinterpret_cast<const float4*>(lds + rr * kLines + 4 * q);
            if (TEST) {
                float* d = a.dst + (int64_t)r * a.dst_stride + c;
                const float out = nodata();
                if (non_ground(A[u].x, o.x, a.t)) d[0] = out;
                if (c + 1 < a.w && non_ground(A[u].y, o.y, a.t)) d[1] = out;
                if (c + 2 < a.w && non_ground(A[u].z, o.z, a.t)) d[2] = out;
                if (c + 3 < a.w && non_ground(A[u].w, o.w, a.t)) d[3] = out;
                if (!a.out) continue;                            // the last level: nobody reads Ok
            }
            *reinterpret_cast<pcr_f4v*>(a.out + (int64_t)r * a.out_stride + c) = pcr_f4v{o.x, o.y, o.z, o.w};
        }
    }
}

struct DiffArgs {
    const float* top;
    const float* gnd;
    float* dst;
    int w, h;
    int64_t top_stride, gnd_stride, dst_stride;
};

template <bool VEC>
__global__ __launch_bounds__(256) void k_band_difference(const DiffArgs a) {
    const int c = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (c >= a.w) return;
    for (int r = blockIdx.y; r < a.h; r += gridDim.y) {
        const float4 t = load_quad<VEC>(a.top + (int64_t)r * a.top_stride, c, a.w);
        const float4 g = load_quad<VEC>(a.gnd + (int64_t)r * a.gnd_stride, c, a.w);
        float* d = a.dst + (int64_t)r * a.dst_stride + c;
        if (VEC && c + 4 <= a.w) {
            __builtin_nontemporal_store(pcr_f4v{difference(t.x, g.x), difference(t.y, g.y), difference(t.z, g.z), difference(t.w, g.w)},
                                        reinterpret_cast<pcr_f4v*>(d));
        } else {
            d[0] = difference(t.x, g.x);
            if (c + 1 < a.w) d[1] = difference(t.y, g.y);
            if (c + 2 < a.w) d[2] = difference(t.z, g.z);
            if (c + 3 < a.w) d[3] = difference(t.w, g.w);
        }
    }
}

int64_t work_pitch(int width) { return ((int64_t)width + 3) & ~(int64_t)3; }
size_t work_bytes_of(int width, int height) { return (size_t)3 * (size_t)work_pitch(width) * (size_t)height * 4 + 16; }

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" int pcr_hip_ground_filter_work_bytes(int width, int height, size_t* bytes) {
    if (int rc = band::check_extent("ground_filter_work_bytes", bytes != nullptr, width, height)) return rc;
    *bytes = work_bytes_of(width, height);
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_ground_filter(const float* src, float* dst, int width, int height, int64_t src_stride, int64_t dst_stride,
                                     int levels, const int* radii, const float* thresholds, void* d_work, size_t work_bytes,
                                     pcr_hip_stream s) {
    if (int rc = band::check_bands("ground_filter", width, height, {{"src", src, src_stride}, {"dst", dst, dst_stride}},
                                   radii && thresholds && d_work)) return rc;
    PCR_REQUIRE(levels >= 1 && levels <= ground::kMaxLevels, "ground_filter: levels must be between 1 and 64");
    for (int k = 0; k < levels; ++k) {
        PCR_REQUIRE(radii[k] >= 1 && radii[k] <= ground::kMaxRadius, "ground_filter: a radius must be between 1 and 64");
        PCR_REQUIRE(k == 0 || radii[k] > radii[k - 1], "ground_filter: radii must be strictly increasing");
        PCR_REQUIRE(thresholds[k] >= 0.0f && thresholds[k] <= FLT_MAX, "ground_filter: a threshold must be finite and not negative");
    }
    PCR_REQUIRE(work_bytes >= work_bytes_of(width, height), "ground_filter: work_bytes too small (pcr_hip_ground_filter_work_bytes)");
    {
        const band::Span sb = band::span_of(src, width, height, src_stride), db = band::span_of(dst, width, height, dst_stride);
        const band::Span wb = band::span_of(d_work, work_bytes);
        PCR_REQUIRE(!band::overlap(sb, db), "ground_filter: dst overlaps src");
        PCR_REQUIRE(!band::overlap(sb, wb), "ground_filter: the workspace overlaps src");
        PCR_REQUIRE(!band::overlap(db, wb), "ground_filter: the workspace overlaps dst");
    }
    if (int rc = band::check_tile_rows("ground_filter", height, kLines)) return rc;

    const int64_t pitch = work_pitch(width);
    float* base = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(d_work) + 15) & ~(uintptr_t)15);
    float* A = base;
    float* T1 = base + pitch * height;
    float* T2 = base + 2 * pitch * height;
    hipStream_t st = static_cast<hipStream_t>(s);
    const dim3 grid_rows((width + kTile - 1) / kTile, (height + kLines - 1) / kLines);
    const dim3 grid_cols((width + kLines - 1) / kLines, (height + kTile - 1) / kTile);

    for (int k = 0; k < levels; ++k) {
        const int R = radii[k];
        const size_t lds_rows = (size_t)kLines * (kTile + 2 * ((R + 3) & ~3) + 1) * 4;
        const size_t lds_cols = (size_t)kLines * (kTile + 2 * R) * 4;
        PassArgs a{};
        a.w = width;
        a.h = height;
        a.R = R;
        a.t = thresholds[k];
        // row-erode: A(k-1) -> T1 (level 1: src, which dst gets a cleaned copy of)
        a.in = k == 0 ? src : A;
        a.in_stride = k == 0 ? src_stride : pitch;
        a.out = T1;
        a.out_stride = pitch;
        a.dst = k == 0 ? dst : nullptr;
        a.dst_stride = dst_stride;
        a.dst_vec = aligned16(dst, dst_stride);
        if (aligned16(a.in, a.in_stride)) hipLaunchKernelGGL((k_ground_rows<false, true>), grid_rows, dim3(kLines), lds_rows, st, a);
        else hipLaunchKernelGGL((k_ground_rows<false, false>), grid_rows, dim3(kLines), lds_rows, st, a);
        // column-erode: T1 -> T2
        a.in = T1;
        a.in_stride = pitch;
        a.out = T2;
        a.dst = nullptr;
        hipLaunchKernelGGL((k_ground_cols<false, false>), grid_cols, dim3(kLines), lds_cols, st, a);
        // row-dilate: T2 -> T1
        a.in = T2;
        a.out = T1;
        hipLaunchKernelGGL((k_ground_rows<true, true>), grid_rows, dim3(kLines), lds_rows, st, a);
        // column-dilate: T1 -> Ok, tested against A(k-1) and stored over it
        a.in = T1;
        a.a_in = k == 0 ? src : A;
        a.a_stride = k == 0 ? src_stride : pitch;
        a.a_vec = aligned16(a.a_in, a.a_stride);
        a.out = k + 1 < levels ? A : nullptr;
        a.dst = dst;
        hipLaunchKernelGGL((k_ground_cols<true, true>), grid_cols, dim3(kLines), lds_cols, st, a);
    }
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}

extern "C" int pcr_hip_band_difference(const float* top, const float* ground, float* dst, int width, int height, int64_t top_stride,
                                       int64_t ground_stride, int64_t dst_stride, pcr_hip_stream s) {
    if (int rc = band::check_bands("band_difference", width, height,
                                   {{"top", top, top_stride}, {"ground", ground, ground_stride}, {"dst", dst, dst_stride}})) return rc;
    DiffArgs a;
    a.top = top;
    a.gnd = ground;
    a.dst = dst;
    a.w = width;
    a.h = height;
    a.top_stride = top_stride;
    a.gnd_stride = ground_stride;
    a.dst_stride = dst_stride;
    const dim3 grid((width + 1023) / 1024, height < 65535 ? height : 65535);
    hipStream_t st = static_cast<hipStream_t>(s);
    if (aligned16(top, top_stride) && aligned16(ground, ground_stride) && aligned16(dst, dst_stride))
        hipLaunchKernelGGL((k_band_difference<true>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((k_band_difference<false>), grid, dim3(256), 0, st, a);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}
