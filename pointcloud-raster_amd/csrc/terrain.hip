// terrain.hip -- pcr_hip_terrain: slope, aspect, hillshade, TRI, TPI and roughness of one band (the contract: terrain.hpp),
// every product asked for in one launch that reads the source once.
//
// One workgroup of 256 lanes owns a 64 x 32 tile of the band; lane (lx, ly) of its 16 x 16 owns the four cells at column 4 lx
// of tile rows ly and ly + 16.
//   1  the tile goes to LDS with a 1-cell apron: the body as one quad per lane and tile half (16-byte loads; the scalar
//      variant serves rows that do not start on 16 bytes), the rows above and below as 32 quads, the columns left and right as
//      68 single cells, all in the same pass; cells outside the image as NaN.  The apron's lines are the neighbour tiles'
//      body: they come from L2.  LDS: 34 rows x 72 floats = 9.6 KB.
//   2  a lane reads its quad's 3 x 6 window from LDS and evaluates the four cells with the contract's lines, in binary64.
//   3  every product asked for leaves as one 16-byte non-temporal store per quad (scalar stores in the scalar variant and for
//      the quad that the image's right edge cuts).
// The product mask is a kernel argument (wave-uniform: scalar branches); the instantiation is picked by CLASS -- whether any
// product of p and q is asked for, whether any of the nine values themselves -- so that sqrt, division and atan_deg are not in
// the code of a launch that needs none of them.  Every cell of every dst is stored exactly once; src is only read; no
// atomics, no scratch.
#include "band_pass.hpp"
#include "terrain.hpp"

#include <cmath>

namespace pcrhip {
namespace {

using namespace terrain;

constexpr int kTileW = 64, kTileH = 32;
constexpr int kPitch = kTileW + 8;                               // image column c0 - 1 is LDS column 3: the body's quads stay aligned
constexpr int kRows = kTileH + 2;

struct TerrainArgs {
    const float* src;
    int w, h;
    int64_t src_stride;
    float* dst[kProducts];                                       // by product id; null: not asked for
    int64_t dst_stride[kProducts];
    unsigned mask;
    int edges;
    Consts k;
};

template <bool VEC, bool HORN, bool RUGGED>
__global__ __launch_bounds__(256) void k_terrain(const TerrainArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[kRows * kPitch];
    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    const int c0 = blockIdx.x * kTileW, r0 = blockIdx.y * kTileH;
    const int c = c0 + 4 * lx;
    const float out = nodata();

    // 1: the body ...
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + ly + 16 * p;
        float4 x = make_float4(out, out, out, out);
        if (r < a.h) {
            const float* row = a.src + (int64_t)r * a.src_stride;
            if (VEC && c + 4 <= a.w) {
                x = *reinterpret_cast<const float4*>(row + c);
            } else {
                if (c < a.w) x.x = row[c];
                if (c + 1 < a.w) x.y = row[c + 1];
                if (c + 2 < a.w) x.z = row[c + 2];
                if (c + 3 < a.w) x.w = row[c + 3];
            }
        }
        *reinterpret_cast<float4*>(&tile[(1 + ly + 16 * p) * kPitch + 4 + 4 * lx]) = x;
    }
    // ... and the apron: lanes 0..31 the quads of the rows above and below, lanes 32..99 the cells left and right
    if (tid < 32) {
        const int below = tid >> 4, gc = c0 + 4 * (tid & 15);
        const int r = below ? r0 + kTileH : r0 - 1;
        float4 x = make_float4(out, out, out, out);
        if (r >= 0 && r < a.h) {
            const float* row = a.src + (int64_t)r * a.src_stride;
            if (VEC && gc + 4 <= a.w) {
                x = *reinterpret_cast<const float4*>(row + gc);
            } else {
                if (gc < a.w) x.x = row[gc];
                if (gc + 1 < a.w) x.y = row[gc + 1];
                if (gc + 2 < a.w) x.z = row[gc + 2];
                if (gc + 3 < a.w) x.w = row[gc + 3];
            }
        }
        *reinterpret_cast<float4*>(&tile[(below ? kRows - 1 : 0) * kPitch + 4 + 4 * (tid & 15)]) = x;
    } else if (tid < 32 + 2 * kRows) {
        const int j = tid - 32, right = j & 1, lr = j >> 1;
        const int r = r0 - 1 + lr, gc = right ? c0 + kTileW : c0 - 1;
        float x = out;
        if (r >= 0 && r < a.h && gc >= 0 && gc < a.w) x = a.src[(int64_t)r * a.src_stride + gc];
        tile[lr * kPitch + (right ? 4 + kTileW : 3)] = x;
    }
    __syncthreads();

    // 2, 3
    if (c >= a.w) return;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + ly + 16 * p;
        if (r >= a.h) continue;
        const float* t = &tile[(ly + 16 * p) * kPitch + 3 + 4 * lx];      // cell a of the quad's first cell
        float v[3][6];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float4 m = *reinterpret_cast<const float4*>(t + d * kPitch + 1);
            v[d][0] = t[d * kPitch];
            v[d][1] = m.x; v[d][2] = m.y; v[d][3] = m.z; v[d][4] = m.w;
            v[d][5] = t[d * kPitch + 5];
        }
        float res[kProducts][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float w9[9] = {v[0][j], v[0][j + 1], v[0][j + 2], v[1][j], v[1][j + 1], v[1][j + 2], v[2][j], v[2][j + 1], v[2][j + 2]};
            float o[kProducts] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            const bool ok = window(w9, a.edges);
            evaluate<HORN, RUGGED>(w9, ok, a.mask, a.k, o);
#pragma unroll
            for (int n = 0; n < kProducts; ++n) res[n][j] = o[n];
        }
#pragma unroll
        for (int n = 0; n < kProducts; ++n) {
            if (!(((HORN ? kHornMask : 0u) | (RUGGED ? kRuggedMask : 0u)) & (1u << n)) || !(a.mask & (1u << n))) continue;
            float* row = a.dst[n] + (int64_t)r * a.dst_stride[n] + c;
            if (VEC && c + 4 <= a.w) {
                __builtin_nontemporal_store(pcr_f4v{res[n][0], res[n][1], res[n][2], res[n][3]}, reinterpret_cast<pcr_f4v*>(row));
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c + j < a.w) __builtin_nontemporal_store(res[n][j], row + j);
            }
        }
    }
}

template <bool VEC>
void launch(const TerrainArgs& a, dim3 grid, hipStream_t st) {
    const bool horn = a.mask & kHornMask, rugged = a.mask & kRuggedMask;
    if (horn && rugged) hipLaunchKernelGGL((k_terrain<VEC, true, true>), grid, dim3(256), 0, st, a);
    else if (horn) hipLaunchKernelGGL((k_terrain<VEC, true, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_terrain<VEC, false, true>), grid, dim3(256), 0, st, a);
}

}  // namespace
}  // namespace pcrhip

using namespace pcrhip;

extern "C" int pcr_hip_terrain(const float* src, int width, int height, int64_t src_stride, int n_products, const int* products,
                               float* const* dsts, const int64_t* dst_strides, double cell_size_x, double cell_size_y,
                               double z_factor, int edges, double sin_alt, double ls, double lc, pcr_hip_stream s) {
    const std::string fn = "terrain";
    if (int rc = band::check_extent(fn, src && products && dsts && dst_strides, width, height)) return rc;
    PCR_REQUIRE(n_products >= 1 && n_products <= terrain::kProducts, "terrain: n_products must be between 1 and 7");
    TerrainArgs a{};
    for (int n = 0; n < n_products; ++n) {
        PCR_REQUIRE(products[n] >= 0 && products[n] < terrain::kProducts, "terrain: unknown product");
        PCR_REQUIRE(!(a.mask & (1u << products[n])), "terrain: duplicate product");
        PCR_REQUIRE(dsts[n], "terrain: null argument");
        a.mask |= 1u << products[n];
        a.dst[products[n]] = dsts[n];
        a.dst_stride[products[n]] = dst_strides[n];
    }
    if (int rc = band::check_stride(fn, "src", src_stride, width)) return rc;
    for (int n = 0; n < n_products; ++n)
        if (int rc = band::check_stride(fn, "dst", dst_strides[n], width)) return rc;
    PCR_REQUIRE(std::isfinite(cell_size_x) && cell_size_x != 0.0 && std::isfinite(cell_size_y) && cell_size_y != 0.0,
                "terrain: cell sizes must be finite and not zero");
    PCR_REQUIRE(std::isfinite(z_factor) && z_factor != 0.0, "terrain: z_factor must be finite and not zero");
    PCR_REQUIRE(edges == 0 || edges == 1, "terrain: edges must be 0 or 1");
    PCR_REQUIRE(std::isfinite(sin_alt) && std::isfinite(ls) && std::isfinite(lc), "terrain: the light constants must be finite");
    const band::Span from = band::span_of(src, width, height, src_stride);
    bool vec = band::aligned16(src, src_stride);
    for (int n = 0; n < n_products; ++n) {
        const band::Span to = band::span_of(dsts[n], width, height, dst_strides[n]);
        PCR_REQUIRE(!band::overlap(from, to), "terrain: dst overlaps src");
        for (int m = 0; m < n; ++m)
            PCR_REQUIRE(!band::overlap(to, band::span_of(dsts[m], width, height, dst_strides[m])), "terrain: dst overlaps another dst");
        vec = vec && band::aligned16(dsts[n], dst_strides[n]);
    }
    if (int rc = band::check_tile_rows(fn, height, kTileH)) return rc;
    a.src = src;
    a.w = width;
    a.h = height;
    a.src_stride = src_stride;
    a.edges = edges;
    a.k.kx = terrain::scale(z_factor, 8.0, cell_size_x);
    a.k.ky = terrain::scale(z_factor, -8.0, cell_size_y);
    a.k.sin_alt = sin_alt;
    a.k.ls = ls;
    a.k.lc = lc;
    const dim3 grid((width + kTileW - 1) / kTileW, (height + kTileH - 1) / kTileH);
    hipStream_t st = static_cast<hipStream_t>(s);
    if (vec) launch<true>(a, grid, st);
    else launch<false>(a, grid, st);
    PCR_HIP_TRY(hipGetLastError());
    return PCR_HIP_OK;
}
