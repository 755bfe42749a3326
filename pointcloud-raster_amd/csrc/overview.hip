// overview.hip -- pcr_hip_downsample2: the overview pyramid of one band, up to six levels per read of the source.
//
// One workgroup of 256 lanes owns a 64x64 source tile; lane (lx, ly) of its 16x16 owns the 4x4 block at (4 lx, 4 ly).
//   level 0   four 16-byte loads per lane; the 16 lanes of a tile row read 256 contiguous bytes (non-temporal: read once)
//   level 1   the lane's 2x2, in registers; two 8-byte stores per lane, 128 contiguous bytes per row of 16 lanes
//   level 2   the lane's one cell, in registers; one 4-byte store, 64 contiguous bytes per row of 16 lanes
//   level 3-6 8x8, 4x4, 2x2, 1 cells of the tile, each made from the level before it through LDS (a barrier per level)
// A 64-aligned tile holds every 2x2 window of levels 1..6 whole, so workgroups never meet: no atomics, no hand-off.  More than
// six levels: the launch function starts the kernel again on level 6, 12, ... on the same stream.  Cells outside the source are
// NaN (invalid, overview.hpp); a level cell outside its level is computed and never stored.
// The scalar variant (VEC = false) serves rows that do not start on 16 bytes.
#include "band_pass.hpp"
#include "overview.hpp"

namespace pcrhip {
namespace {

using namespace overview;

struct Down2Args {
    const float* src;
    int w, h;
    int64_t stride;
    float* dst[kLevelsPerPass];
    int levels;                 // 1..kLevelsPerPass
    int mode;
    int pair_stores;            // level 1: rows start on 8 bytes
};

template <bool VEC>
__global__ __launch_bounds__(256) void k_downsample2(const Down2Args a) {
    __shared__ float lds[16 * 16 + 8 * 8 + 4 * 4 + 2 * 2 + 1];       // levels 2..6 of the tile
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int c0 = blockIdx.x * kTile + lx * 4, r0 = blockIdx.y * kTile + ly * 4;
    const float out = nodata();

    float v[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + i;
        const float* row = a.src + (int64_t)r * a.stride;
        if (VEC && r < a.h && c0 + 4 <= a.w) {
            const float4 q = stream_load(reinterpret_cast<const float4*>(row + c0));
            v[i][0] = q.x; v[i][1] = q.y; v[i][2] = q.z; v[i][3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i][j] = (r < a.h && c0 + j < a.w) ? row[c0 + j] : out;
        }
    }

    // level 1
    const int w1 = level_extent(a.w, 1), h1 = level_extent(a.h, 1);
    float l1[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
            l1[i][j] = down4(a.mode, v[2 * i][2 * j], v[2 * i][2 * j + 1], v[2 * i + 1][2 * j], v[2 * i + 1][2 * j + 1]);
        const int r = blockIdx.y * (kTile / 2) + ly * 2 + i, c = blockIdx.x * (kTile / 2) + lx * 2;
        if (r < h1) {
            float* p = a.dst[0] + (int64_t)r * w1 + c;
            if (a.pair_stores && c + 2 <= w1) *reinterpret_cast<float2*>(p) = make_float2(l1[i][0], l1[i][1]);
            else {
                if (c < w1) p[0] = l1[i][0];
                if (c + 1 < w1) p[1] = l1[i][1];
            }
        }
    }
    if (a.levels < 2) return;                                   // uniform: no barrier has been passed

    // level 2
    const float l2 = down4(a.mode, l1[0][0], l1[0][1], l1[1][0], l1[1][1]);
    {
        const int w2 = level_extent(a.w, 2), h2 = level_extent(a.h, 2);
        const int r = blockIdx.y * (kTile / 4) + ly, c = blockIdx.x * (kTile / 4) + lx;
        if (r < h2 && c < w2) a.dst[1][(int64_t)r * w2 + c] = l2;
    }
    lds[threadIdx.x] = l2;

    // levels 3..6: n x n cells from the 2n x 2n of the level before
    float* prev = lds;
    int n = 8;
    for (int k = 3; k <= a.levels; ++k, n >>= 1) {              // a.levels is uniform: every lane meets every barrier
        __syncthreads();
        float* cur = prev + 4 * n * n;
        if ((int)threadIdx.x < n * n) {
            const int y = threadIdx.x / n, x = threadIdx.x % n;
            const float* q = prev + (2 * y) * (2 * n) + 2 * x;
            const float val = down4(a.mode, q[0], q[1], q[2 * n], q[2 * n + 1]);
            cur[threadIdx.x] = val;
            const int wk = level_extent(a.w, k), hk = level_extent(a.h, k);
            const int r = blockIdx.y * n + y, c = blockIdx.x * n + x;
            if (r < hk && c < wk) a.dst[k - 1][(int64_t)r * wk + c] = val;
        }
        prev = cur;
    }
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" int pcr_hip_downsample2(const float* src, int width, int height, int64_t src_stride, float* const* dst, int levels,
                                   int mode, pcr_hip_stream s) {
    if (int rc = band::check_extent("downsample2", src && dst, width, height)) return rc;
    PCR_REQUIRE(levels > 0, "downsample2: levels must be positive");
    if (int rc = band::check_stride("downsample2", "src", src_stride, width)) return rc;
    PCR_REQUIRE(mode == overview::kAverage || mode == overview::kNearest, "downsample2: unknown mode (0 average, 1 nearest)");
    PCR_REQUIRE(levels <= overview::max_levels(width, height), "downsample2: more levels than halvings down to 1x1");
    for (int k = 0; k < levels; ++k) PCR_REQUIRE(dst[k], "downsample2: null level pointer");
    if (int rc = band::check_tile_rows("downsample2", height, overview::kTile)) return rc;
    hipStream_t st = static_cast<hipStream_t>(s);
    int w = width, h = height;
    int64_t stride = src_stride;
    for (int done = 0; done < levels; done += overview::kLevelsPerPass) {
        Down2Args a;
        a.src = src;
        a.w = w;
        a.h = h;
        a.stride = stride;
        a.levels = levels - done < overview::kLevelsPerPass ? levels - done : overview::kLevelsPerPass;
        a.mode = mode;
        for (int k = 0; k < overview::kLevelsPerPass; ++k) a.dst[k] = k < a.levels ? dst[done + k] : nullptr;
        a.pair_stores = overview::level_extent(w, 1) % 2 == 0 && (reinterpret_cast<uintptr_t>(a.dst[0]) & 7) == 0;
        const bool vec = band::aligned16(src, stride);
        const dim3 grid((w + overview::kTile - 1) / overview::kTile, (h + overview::kTile - 1) / overview::kTile);
        if (vec) hipLaunchKernelGGL(k_downsample2<true>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_downsample2<false>, grid, dim3(256), 0, st, a);
        PCR_HIP_TRY(hipGetLastError());
        if (a.levels == overview::kLevelsPerPass) {              // the next pass reads the last level written
            src = dst[done + overview::kLevelsPerPass - 1];
            w = overview::level_extent(w, overview::kLevelsPerPass);
            h = overview::level_extent(h, overview::kLevelsPerPass);
            stride = w;
        }
    }
    return PCR_HIP_OK;
}
