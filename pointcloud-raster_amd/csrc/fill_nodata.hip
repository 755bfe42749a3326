// fill_nodata.hip -- pcr_hip_fill_nodata: the NaN cells of one band filled from their valid neighbours within a radius
// (the contract: fill_nodata.hpp), out of place.
//
// One workgroup of 256 lanes owns a 64 x 32 tile of the band; lane (lx, ly) of its 16 x 16 owns the four cells at column 4 lx
// of tile rows ly and ly + 16.
//   1  every lane loads its two quads (16-byte non-temporal loads; the scalar variant serves rows that do not start on 16
//      bytes) and the tile's NaN cells are counted: one ballot per quad element and wave, the four waves' counts meet in LDS.
//   2  a tile without a NaN -- the typical tile -- is stored from the registers and the workgroup is done: no apron is
//      read, nothing is staged.
//   3  otherwise the cells that are not NaN are stored from the registers, and the NaN cells are compacted into a list in LDS
//      (rank = the lane's position in the ballot, base = the waves' counts).  The tile and its apron of R cells go to LDS once:
//      the tile from the registers, the apron from the band (cached loads: the neighbours' workgroups read the same lines),
//      cells outside the image as NaN.  The weights 1 / d2 and the disc's half width per window row are computed once per
//      workgroup into LDS with the contract's division.
//   4  list entries are dealt to the lanes round robin.  A lane walks its cell's window in LDS in the contract's order with
//      binary64 sums and stores the result itself.  The cost follows the number of holes: a lane never waits on a fixed
//      cell's neighbour.
// Every cell of dst is stored exactly once, non-temporally; src is only read; no atomics, no scratch.
// LDS is sized by the radius class RMAX (8, 16, 32: the smallest that holds R), because the LDS a workgroup reserves decides
// how many hole-free tiles a CU copies at a time: (32 + 2 RMAX) rows x (64 + 2 RMAX) floats + the list (4 KB) + the weights
// = 19.8 / 29.9 / 57.8 KB, i.e. 8 / 5 / 2 workgroups per CU.
#include "band_pass.hpp"
#include "fill_nodata.hpp"

namespace pcrhip {
namespace {

using namespace fill;

constexpr int kTileW = 64, kTileH = 32;

struct FillArgs {
    const float* src;
    float* dst;
    int w, h;
    int64_t src_stride, dst_stride;
    int R;
};

template <bool VEC, int RMAX>                                    // a.R <= RMAX, RMAX a multiple of 4
__global__ __launch_bounds__(256) void k_fill_nodata(const FillArgs a) {
    constexpr int kPitch = kTileW + 2 * RMAX;                    // the tile and an apron rounded up to whole quads
    constexpr int kRows = kTileH + 2 * RMAX;
    __shared__ __attribute__((aligned(16))) float tile[kRows * kPitch];
    __shared__ unsigned short holes[kTileW * kTileH];           // row in tile << 6 | column in tile
    __shared__ float wt[(RMAX + 1) * (RMAX + 1)];               // [|dr| * (R + 1) + |dc|]
    __shared__ int half[RMAX + 1];
    __shared__ int wave_holes[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lx = tid & 15, ly = tid >> 4;
    const int c0 = blockIdx.x * kTileW, r0 = blockIdx.y * kTileH;
    const int c = c0 + 4 * lx;
    const float out = nodata();

    // 1: the lane's two quads; inside: bit 4 p + j = cell j of quad p is a cell of the image
    float v[2][4];
    unsigned inside = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + ly + 16 * p;
        const float* row = a.src + (int64_t)r * a.src_stride;
        if (VEC && r < a.h && c + 4 <= a.w) {
            const float4 q = stream_load(reinterpret_cast<const float4*>(row + c));
            v[p][0] = q.x; v[p][1] = q.y; v[p][2] = q.z; v[p][3] = q.w;
            inside |= 0xFu << (4 * p);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = r < a.h && c + j < a.w;
                v[p][j] = in ? row[c + j] : out;
                inside |= (unsigned)in << (4 * p + j);
            }
        }
    }
    int rank[2][4];                                              // position of the lane's NaN cells among its wave's
    int mine = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool hole = ((inside >> (4 * p + j)) & 1u) && v[p][j] != v[p][j];
            const unsigned long long m = __ballot(hole);
            rank[p][j] = mine + __popcll(m & ((1ull << lane) - 1ull));
            mine += __popcll(m);                                 // (wave-uniform: the wave's count so far)
        }
    if (lane == 0) wave_holes[wave] = mine;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = wave_holes[k];
        base += k < wave ? n : 0;
        total += n;
    }

    // 2, and the first half of 3: the cells that are not NaN leave from the registers
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + ly + 16 * p;
        float* row = a.dst + (int64_t)r * a.dst_stride;
        const unsigned in4 = (inside >> (4 * p)) & 0xFu;
        const bool whole = v[p][0] == v[p][0] && v[p][1] == v[p][1] && v[p][2] == v[p][2] && v[p][3] == v[p][3];
        if (VEC && in4 == 0xFu && whole) {
            __builtin_nontemporal_store(pcr_f4v{v[p][0], v[p][1], v[p][2], v[p][3]}, reinterpret_cast<pcr_f4v*>(row + c));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (((in4 >> j) & 1u) && v[p][j] == v[p][j]) __builtin_nontemporal_store(v[p][j], row + c + j);
        }
    }
    if (total == 0) return;                                      // uniform: wave_holes is the same for every lane

    // 3: the list, the weights, the tile and its apron
    const int R = a.R, Ra = (R + 3) & ~3;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (((inside >> (4 * p + j)) & 1u) && v[p][j] != v[p][j])
                holes[base + rank[p][j]] = (unsigned short)(((ly + 16 * p) << 6) | (4 * lx + j));
    for (int i = tid; i < (R + 1) * (R + 1); i += 256) {
        const int dr = i / (R + 1), dc = i % (R + 1);
        wt[i] = i ? weight(dr * dr + dc * dc) : 0.0f;
    }
    if (tid <= R) half[tid] = half_width(R, tid);
#pragma unroll
    for (int p = 0; p < 2; ++p)
        *reinterpret_cast<float4*>(&tile[(R + ly + 16 * p) * kPitch + Ra + 4 * lx]) = make_float4(v[p][0], v[p][1], v[p][2], v[p][3]);
    {
        // window rows r0 - R .. r0 + 32 + R - 1 at LDS rows 0 ..; window columns c0 - Ra .. c0 + 64 + Ra - 1 in quads
        const int quads = (kTileW + 2 * Ra) / 4, rows = kTileH + 2 * R;
        for (int i = tid; i < quads * rows; i += 256) {
            const int lr = i / quads, q = i % quads;
            const int r = r0 - R + lr, gc = c0 - Ra + 4 * q;
            if (r >= r0 && r < r0 + kTileH && gc >= c0 && gc < c0 + kTileW) continue;      // the tile itself
            float4 x = make_float4(out, out, out, out);
            if (r >= 0 && r < a.h) {                             // (band::load_quad by hand: the compiler schedules the call otherwise)
                const float* row = a.src + (int64_t)r * a.src_stride;
                if (VEC && gc >= 0 && gc + 4 <= a.w) {
                    x = *reinterpret_cast<const float4*>(row + gc);
                } else {
                    if (gc >= 0 && gc < a.w) x.x = row[gc];
                    if (gc + 1 >= 0 && gc + 1 < a.w) x.y = row[gc + 1];
                    if (gc + 2 >= 0 && gc + 2 < a.w) x.z = row[gc + 2];
                    if (gc + 3 >= 0 && gc + 3 < a.w) x.w = row[gc + 3];
                }
            }
            *reinterpret_cast<float4*>(&tile[lr * kPitch + 4 * q]) = x;
        }
    }
    __syncthreads();

    // 4: one list entry per lane and turn; the window of tile cell (tr, tc) is centred on LDS cell (R + tr, Ra + tc)
    for (int i = tid; i < total; i += 256) {
        const int code = holes[i], tr = code >> 6, tc = code & 63;
        const float* centre = &tile[(R + tr) * kPitch + Ra + tc];
        double s = 0.0, t = 0.0;
        for (int dr = -R; dr <= R; ++dr) {
            const int ar = dr < 0 ? -dr : dr, hw = half[ar];
            const float* wrow = wt + ar * (R + 1);
            const float* trow = centre + dr * kPitch;
            for (int dc = -hw; dc <= hw; ++dc) {
                const float x = trow[dc];
                if (x != x || (dr | dc) == 0) continue;
                accumulate(s, t, wrow[dc < 0 ? -dc : dc], x);
            }
        }
        __builtin_nontemporal_store(finish(s, t, *centre), a.dst + (int64_t)(r0 + tr) * a.dst_stride + c0 + tc);
    }
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" int pcr_hip_fill_nodata(const float* src, float* dst, int width, int height, int64_t src_stride, int64_t dst_stride,
                                   int radius, pcr_hip_stream s) {
    if (int rc = band::check_bands("fill_nodata", width, height, {{"src", src, src_stride}, {"dst", dst, dst_stride}})) return rc;
    PCR_REQUIRE(radius >= 1 && radius <= fill::kMaxRadius, "fill_nodata: radius must be between 1 and 32");
    // (the fill reads src after it has stored dst cells)
    PCR_REQUIRE(!band::overlap(band::span_of(src, width, height, src_stride), band::span_of(dst, width, height, dst_stride)),
                "fill_nodata: dst overlaps src");
    if (int rc = band::check_tile_rows("fill_nodata", height, kTileH)) return rc;
    FillArgs a;
    a.src = src;
    a.dst = dst;
    a.w = width;
    a.h = height;
    a.src_stride = src_stride;
    a.dst_stride = dst_stride;
    a.R = radius;
    const bool vec = band::aligned16(src, src_stride) && band::aligned16(dst, dst_stride);
    const dim3 grid((width + kTileW - 1) / kTileW, (height + kTileH - 1) / kTileH);
    hipStream_t st = static_cast<hipStream_t>(s);
    if (radius <= 8) {
        if (vec) hipLaunchKernelGGL((k_fill_nodata<true, 8>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_fill_nodata<false, 8>), grid, dim3(256), 0, st, a);
    } else if (radius <= 16) {
        if (vec) hipLaunchKernelGGL((k_fill_nodata<true, 16>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_fill_nodata<false, 16>), grid, dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((k_fill_nodata<true, fill::kMaxRadius>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((k_fill_nodata<false, fill::kMaxRadius>), grid, dim3(256), 0, st, a);
    }
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}
