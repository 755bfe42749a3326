// band_pass.hpp -- what the kernels over one strided band share (fill_nodata.hip, ground_filter.hip, overview.hip): the checks
// their entry points start with, the bytes a band spans (the zonal folds' too: zone_fold.hpp), the alignment that picks a VEC
// variant, and the quad load.
#pragma once

#include "common.hpp"

#include <initializer_list>

namespace pcrhip {
namespace band {

// The rows of a band start on 16 bytes: what a kernel's VEC variant (16-byte accesses) asks of every band it is used on.
inline bool aligned16(const void* p, int64_t stride) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && stride % 4 == 0; }

// [b, e): the bytes a band of `height` rows of `width` elements (floats, unless `elem` says otherwise) `stride` apart spans, first
// cell to last; or `bytes` at p.
struct Span { uintptr_t b, e; };
inline Span span_of(const void* p, int width, int height, int64_t stride, size_t elem = 4) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(p);
    return {b, b + ((uintptr_t)(height - 1) * (uintptr_t)stride + (uintptr_t)width) * elem};
}
inline Span span_of(const void* p, size_t bytes) { return {reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes}; }
// An empty span overlaps nothing (the point folds' inputs when there is no point).  The band kernels never pass one: width, height
// and Z are at least 1 and a work area is refused unless it has its bytes -- rasterize_polygons alone compares first, so a work
// area of no bytes inside its output is refused as too small, not as overlapping.
inline bool overlap(Span x, Span y) { return x.b != x.e && y.b != y.e && !(x.e <= y.b || y.e <= x.b); }

// The checks of entry point `fn`, each PCR_HIP_OK or the failure with fn's message.  check_bands is the usual opening: no null
// pointer (`pointers`: the ones that are no band), a positive extent, then every band's rows at least `width` floats apart.
struct Arg {
    const char* name;                // as the message names its stride: "<name>_stride"
    const void* p;
    int64_t stride;
};
inline int check_extent(const std::string& fn, bool pointers, int width, int height) {
    PCR_REQUIRE(pointers, fn + ": null argument");
    PCR_REQUIRE(width > 0 && height > 0, fn + ": width and height must be positive");
    return PCR_HIP_OK;
}
inline int check_stride(const std::string& fn, const char* name, int64_t stride, int width) {
    PCR_REQUIRE(stride >= width, fn + ": " + name + "_stride smaller than width");
    return PCR_HIP_OK;
}
inline int check_bands(const std::string& fn, int width, int height, std::initializer_list<Arg> bands, bool pointers = true) {
    for (const Arg& a : bands) pointers = pointers && a.p;
    int rc = check_extent(fn, pointers, width, height);
    for (const Arg& a : bands)
        if (rc == PCR_HIP_OK) rc = check_stride(fn, a.name, a.stride, width);
    return rc;
}
// gridDim.y holds the tile rows of a band kernel
inline int check_tile_rows(const std::string& fn, int height, int tile_rows) {
    PCR_REQUIRE((height + tile_rows - 1) / tile_rows <= 65535, fn + ": more than 65535 tile rows");
    return PCR_HIP_OK;
}

#if defined(__HIPCC__)
// cells c .. c + 3 of an image row (null: a row outside the image), cells outside the image as NaN (0x7FC00000)
template <bool VEC>                                              // VEC: the rows start on 16 bytes
__device__ __forceinline__ float4 load_quad(const float* row, int c, int w) {
    const float out = __uint_as_float(0x7FC00000u);
    float4 x = make_float4(out, out, out, out);
    if (!row) return x;
    if (VEC && c >= 0 && c + 4 <= w) return *reinterpret_cast<const float4*>(row + c);
    if (c >= 0 && c < w) x.x = row[c];
    if (c + 1 >= 0 && c + 1 < w) x.y = row[c + 1];
    if (c + 2 >= 0 && c + 2 < w) x.z = row[c + 2];
    if (c + 3 >= 0 && c + 3 < w) x.w = row[c + 3];
    return x;
}
__device__ __forceinline__ float4 load_quad(const float* row, int c, int w, int vec) {
    return vec ? load_quad<true>(row, c, w) : load_quad<false>(row, c, w);
}
#endif  // __HIPCC__

}  // namespace band
}  // namespace pcrhip
